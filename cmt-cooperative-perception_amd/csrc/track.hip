// The multi-object tracker of include/cmt_hip.h on the device:
//   cmt_track_predict: the detections into the tracker's frame with their validity word, the constant-velocity
//                      prediction of every live slot, the live list, the gated squared-distance cost matrix and
//                      the descriptor cmt_lsap reads;
//   cmt_track_update:  matches from cmt_lsap's two tables, the Kalman update per axis, misses and frees, births
//                      into the free slots, the counters and the id of every detection row.
//
// These are latency kernels: a frame has about 100 tracks and 300 boxes, the caps are 512 and 1024.  Everything
// that needs a total order (the live list, the free-slot list, the birth ranks) runs in ONE workgroup of 256
// threads: entry e = it * 256 + tid, so the 64 lanes of a wave hold 64 consecutive entries, a ballot / mbcnt
// gives the rank inside them and an LDS table of at most 16 words the entries before (tile_rank of wave_ops.h).  No atomics:
// the results are bitwise repeatable.  The cost matrix is a launch of its own over tiles of 16 rows x 256
// columns: at the caps it is 512 K elements, 2048 per thread of one workgroup, while as tiles it is one
// short wave of workgroups; it needs the predicted state and the live list complete, which the launch boundary
// gives.  A thread owns a column and keeps its detection in registers over the tile's rows, whose slot, label
// and position are the same in every lane (scalar loads).  Tiles at or beyond n_live rows or n_det columns
// return at once: the counts come from lsap_desc in device memory, the grid is sized by T and D alone.
// The file is built with -ffp-contract=off: every product and sum of the contract is rounded on its own.
#include "box_rigid.h"
#include "wave_ops.h"

constexpr int TRK_THREADS = 256;
constexpr int TRK_T_ITERS = CMT_TRACK_MAX_TRACKS / TRK_THREADS;   // 2
constexpr int TRK_D_ITERS = CMT_TRACK_MAX_DETS / TRK_THREADS;     // 4
constexpr int TRK_ROWS = 16;                                      // rows of a cost tile
static_assert(CMT_TRACK_MAX_TRACKS % TRK_THREADS == 0 && CMT_TRACK_MAX_DETS % TRK_THREADS == 0, "whole passes");

// ---- cmt_track_predict ---------------------------------------------------------------------------------------
struct trp_p {
    float* trk_f;
    int* trk_i;
    const float* det;
    const float* scores;
    const int* labels;
    const int* count;
    const float* gate2;
    float* det_w;
    int* det_ok;
    int* live;
    float* cost;
    long long* desc;
    int T, D, ld, ncls, has_pose;
    float dt, q_pos, q_vel, score_thr, pose_yaw;
    float m[12];
};

__device__ __forceinline__ void trk_predict_axis(float* f, int p, int v, int pp, float dt, float qp, float qv) {
#pragma clang fp contract(off)
    const float Ppp = f[pp], Ppv = f[pp + 1], Pvv = f[pp + 2];
    const float dv = dt * f[v];
    f[p] = f[p] + dv;
    const float dpvv = dt * Pvv;
    const float t1 = Ppv + dpvv;
    const float s = Ppv + t1;
    const float ds = dt * s;
    const float a = Ppp + ds;
    f[pp] = a + qp;
    f[pp + 1] = t1;
    f[pp + 2] = Pvv + qv;
}

__global__ __launch_bounds__(TRK_THREADS) void track_predict_kernel(trp_p p) {
#pragma clang fp contract(off)
    __shared__ int tab[TRK_T_ITERS * 4];
    const int tid = (int)threadIdx.x;
    const int n_det = clamp_count(p.count, p.D);
    for (int j = tid; j < p.D; j += TRK_THREADS) {
        const float* q = p.det + (int64_t)j * p.ld;
        float o[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = q[k];
        if (p.has_pose) {
            float pos[3], vel[2];
            box_rigid(p.m, o[0], o[1], o[2], o[7], o[8], pos, vel);
            o[0] = pos[0], o[1] = pos[1], o[2] = pos[2], o[7] = vel[0], o[8] = vel[1];
            float yaw = o[6] + p.pose_yaw;
            if (yaw >= 3.1415927f) yaw = yaw - 6.2831855f;
            else if (yaw < -3.1415927f) yaw = yaw + 6.2831855f;
            o[6] = yaw;
        }
        bool fin = true;
        float* d = p.det_w + (int64_t)j * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            d[k] = o[k];
            fin = fin && finite32(o[k]);
        }
        const int lab = p.labels[j];
        p.det_ok[j] = (j < n_det && fin && lab >= 0 && lab < p.ncls && p.scores[j] >= p.score_thr) ? 1 : 0;
    }
    const float qp = p.q_pos * p.dt, qv = p.q_vel * p.dt;
    bool alive[TRK_T_ITERS];
    int rank[TRK_T_ITERS];
#pragma unroll
    for (int it = 0; it < TRK_T_ITERS; ++it) {
        const int s = it * TRK_THREADS + tid;
        alive[it] = s < p.T && p.trk_i[s * 8] >= 0;
        if (alive[it]) {
            float* f = p.trk_f + s * 16;
            trk_predict_axis(f, 0, 7, 10, p.dt, qp, qv);
            trk_predict_axis(f, 1, 8, 13, p.dt, qp, qv);
            p.trk_i[s * 8 + 4] += 1;
        }
    }
    const int n_live = tile_rank<TRK_T_ITERS>(alive, rank, tab);
#pragma unroll
    for (int it = 0; it < TRK_T_ITERS; ++it)
        if (alive[it]) p.live[rank[it]] = it * TRK_THREADS + tid;
    if (tid == 0) p.desc[0] = 0, p.desc[1] = n_live, p.desc[2] = n_det, p.desc[3] = p.D;
}

__global__ __launch_bounds__(TRK_THREADS) void track_cost_kernel(trp_p p) {
#pragma clang fp contract(off)
    const int n_live = clamp_index(p.desc[1], p.T), n_det = clamp_index(p.desc[2], p.D);
    const int r0 = (int)blockIdx.y * TRK_ROWS;
    const int j = (int)blockIdx.x * TRK_THREADS + (int)threadIdx.x;
    if (r0 >= n_live || j >= n_det) return;
    const float xj = p.det_w[(int64_t)j * 9], yj = p.det_w[(int64_t)j * 9 + 1];
    const bool ok = p.det_ok[j] != 0;   // then 0 <= lab < ncls
    const int lab = p.labels[j];
    const float gate = ok ? p.gate2[lab] : 0.f;
    const int r1 = r0 + TRK_ROWS < n_live ? r0 + TRK_ROWS : n_live;
    for (int r = r0; r < r1; ++r) {
        const int s = p.live[r];   // written by track_predict_kernel: inside [0, T)
        const float ex = p.trk_f[s * 16] - xj, ey = p.trk_f[s * 16 + 1] - yj;
        const float ex2 = ex * ex, ey2 = ey * ey;
        const float d2 = ex2 + ey2;
        const bool in = ok && lab == p.trk_i[s * 8 + 1] && d2 < gate;
        p.cost[(int64_t)r * p.D + j] = in ? d2 : CMT_TRACK_BIG;
    }
}

// ---- cmt_track_update ----------------------------------------------------------------------------------------
struct tru_p {
    float* trk_f;
    int* trk_i;
    float* hist;
    int* counters;
    const int* live;
    const long long* desc;
    const float* cost;
    const int* match_g;
    const int* match_q;
    const float* det_w;
    const float* scores;
    const int* labels;
    const int* det_ok;
    int* det_track;
    int* det_slot;
    int T, D, H, use_velocity, max_age;
    float r_pos, r_vel, p0_pos, p0_vel, birth_thr;
};

__device__ __forceinline__ void trk_update_axis(float* f, int ip, int iv, int ipp, float zp, float zv, const tru_p& p) {
#pragma clang fp contract(off)
    const float pos = f[ip], vel = f[iv], Ppp = f[ipp], Ppv = f[ipp + 1], Pvv = f[ipp + 2];
    if (p.use_velocity) {
        const float Spp = Ppp + p.r_pos, Spv = Ppv, Svv = Pvv + p.r_vel;
        const float d0 = Spp * Svv, d1 = Spv * Spv;
        const float det = d0 - d1;
        const float a0 = Ppp * Svv, a1 = Ppv * Spv, b0 = Ppv * Spp, b1 = Ppp * Spv;
        const float c0 = Ppv * Svv, c1 = Pvv * Spv, e0 = Pvv * Spp, e1 = Ppv * Spv;
        const float na = a0 - a1, nb = b0 - b1, nc = c0 - c1, ne = e0 - e1;
        const float K00 = na / det, K01 = nb / det, K10 = nc / det, K11 = ne / det;
        const float yp = zp - pos, yv = zv - vel;
        const float u0 = K00 * yp, u1 = K01 * yv, w0 = K10 * yp, w1 = K11 * yv;
        const float du = u0 + u1, dw = w0 + w1;
        f[ip] = pos + du;
        f[iv] = vel + dw;
        const float g0 = K00 * Ppp, g1 = K01 * Ppv, h0 = K00 * Ppv, h1 = K01 * Pvv, k0 = K10 * Ppv, k1 = K11 * Pvv;
        const float g = g0 + g1, h = h0 + h1, k = k0 + k1;
        f[ipp] = Ppp - g;
        f[ipp + 1] = Ppv - h;
        f[ipp + 2] = Pvv - k;
    } else {
        const float S = Ppp + p.r_pos;
        const float K0 = Ppp / S, K1 = Ppv / S;
        const float y = zp - pos;
        const float u = K0 * y, w = K1 * y;
        f[ip] = pos + u;
        f[iv] = vel + w;
        const float g = K0 * Ppp, h = K0 * Ppv, k = K1 * Ppv;
        f[ipp] = Ppp - g;
        f[ipp + 1] = Ppv - h;
        f[ipp + 2] = Pvv - k;
    }
}

__global__ __launch_bounds__(TRK_THREADS) void track_update_kernel(tru_p p) {
#pragma clang fp contract(off)
    __shared__ int tab[TRK_D_ITERS * 4];
    __shared__ int list[CMT_TRACK_MAX_TRACKS];         // the live list, later the free-slot list
    __shared__ int slot_match[CMT_TRACK_MAX_TRACKS];   // the detection matched to a slot or -1
    __shared__ int dslot[CMT_TRACK_MAX_DETS];          // the slot matched to a detection or -1
    const int tid = (int)threadIdx.x;
    const int n_live_in = clamp_index(p.desc[1], p.T), n_det = clamp_index(p.desc[2], p.D);
    const int next_id = p.counters[1], dropped = p.counters[2], frames = p.counters[3];
    bool tf[TRK_T_ITERS];
    int trank[TRK_T_ITERS];
    int id[TRK_T_ITERS];
#pragma unroll
    for (int it = 0; it < TRK_T_ITERS; ++it) {
        const int s = it * TRK_THREADS + tid;
        id[it] = s < p.T ? p.trk_i[s * 8] : -1;
        tf[it] = id[it] >= 0;
        slot_match[s] = -1;
    }
    for (int j = tid; j < CMT_TRACK_MAX_DETS; j += TRK_THREADS) dslot[j] = -1;
    int n_live = tile_rank<TRK_T_ITERS>(tf, trank, tab);
#pragma unroll
    for (int it = 0; it < TRK_T_ITERS; ++it)
        if (tf[it]) list[trank[it]] = it * TRK_THREADS + tid;
    n_live = n_live < n_live_in ? n_live : n_live_in;
    __syncthreads();
    // 1. matches: one writer per detection (match_q[j] == r) and per slot (list is strictly ascending)
    for (int r = tid; r < n_live; r += TRK_THREADS) {
        const int s = list[r];
        if (p.live[r] != s) continue;
        const int j = p.match_g[r];
        if (j < 0 || j >= n_det) continue;
        if (p.match_q[j] != r || p.det_ok[j] == 0) continue;
        if (!(p.cost[(int64_t)r * p.D + j] < CMT_TRACK_BIG)) continue;
        slot_match[s] = j;
        dslot[j] = s;
    }
    __syncthreads();
    // 2., 3. matched and unmatched slots
#pragma unroll
    for (int it = 0; it < TRK_T_ITERS; ++it) {
        const int s = it * TRK_THREADS + tid;
        if (id[it] >= 0) {
            int* ti = p.trk_i + s * 8;
            const int j = slot_match[s];
            if (j >= 0) {
                float* f = p.trk_f + s * 16;
                const float* d = p.det_w + (int64_t)j * 9;
                trk_update_axis(f, 0, 7, 10, d[0], d[7], p);
                trk_update_axis(f, 1, 8, 13, d[1], d[8], p);
#pragma unroll
                for (int k = 2; k < 7; ++k) f[k] = d[k];
                f[9] = p.scores[j];
                ti[2] += 1, ti[3] = 0, ti[5] = j;
                const int hn = ti[6];
                float* h = p.hist + ((int64_t)s * p.H + (int)((unsigned)hn % (unsigned)p.H)) * 3;
                h[0] = f[0], h[1] = f[1], h[2] = d[2];
                ti[6] = hn + 1;
            } else {
                const int misses = ti[3] + 1;
                ti[3] = misses, ti[5] = -1;
                if (misses > p.max_age) ti[0] = id[it] = -1;
            }
        }
        tf[it] = s < p.T && id[it] < 0;
    }
    const int n_free = tile_rank<TRK_T_ITERS>(tf, trank, tab);   // its first barrier: list has been read
#pragma unroll
    for (int it = 0; it < TRK_T_ITERS; ++it)
        if (tf[it]) list[trank[it]] = it * TRK_THREADS + tid;
    // 4. births
    bool df[TRK_D_ITERS];
    int drank[TRK_D_ITERS];
#pragma unroll
    for (int it = 0; it < TRK_D_ITERS; ++it) {
        const int j = it * TRK_THREADS + tid;
        df[it] = j < n_det && p.det_ok[j] != 0 && dslot[j] < 0 && p.scores[j] >= p.birth_thr;
    }
    const int n_born = tile_rank<TRK_D_ITERS>(df, drank, tab);   // its barriers: the free-slot list is written
#pragma unroll
    for (int it = 0; it < TRK_D_ITERS; ++it) {
        const int j = it * TRK_THREADS + tid;
        if (j >= p.D) continue;
        int tr = -1, sl = -1;
        if (df[it]) {
            if (drank[it] < n_free) {
                sl = list[drank[it]];
                tr = next_id + drank[it];
                const float* d = p.det_w + (int64_t)j * 9;
                float* f = p.trk_f + sl * 16;
                int* ti = p.trk_i + sl * 8;
#pragma unroll
                for (int k = 0; k < 7; ++k) f[k] = d[k];
                f[7] = p.use_velocity ? d[7] : 0.f;
                f[8] = p.use_velocity ? d[8] : 0.f;
                f[9] = p.scores[j];
                f[10] = p.p0_pos, f[11] = 0.f, f[12] = p.p0_vel;
                f[13] = p.p0_pos, f[14] = 0.f, f[15] = p.p0_vel;
                ti[0] = tr, ti[1] = p.labels[j], ti[2] = 1, ti[3] = 0, ti[4] = 0, ti[5] = j, ti[6] = 1, ti[7] = 0;
                float* h = p.hist + (int64_t)sl * p.H * 3;
                h[0] = d[0], h[1] = d[1], h[2] = d[2];
            }
        } else if (dslot[j] >= 0) {
            sl = dslot[j];
            tr = p.trk_i[sl * 8];   // a matched slot: no birth writes it
        }
        p.det_track[j] = tr;
        p.det_slot[j] = sl;
    }
    // 5. counters (read into registers before the first barrier)
    if (tid == 0) {
        const int placed = n_born < n_free ? n_born : n_free;
        p.counters[0] = p.T - n_free + placed;
        p.counters[1] = next_id + placed;
        p.counters[2] = dropped + (n_born - placed);
        p.counters[3] = frames + 1;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
extern "C" int64_t cmt_track_predict_args_size(void) { return (int64_t)sizeof(cmt_track_predict_args); }
extern "C" int64_t cmt_track_update_args_size(void) { return (int64_t)sizeof(cmt_track_update_args); }

static inline bool trk_nonneg(float v) { return std::isfinite(v) && v >= 0.f; }
static inline bool trk_pos(float v) { return std::isfinite(v) && v > 0.f; }

extern "C" int cmt_track_predict(const cmt_track_predict_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_track_predict: null argument struct");
    CMT_REQUIRE(a->T >= 1 && a->D >= 1, "cmt_track_predict: T and D must be at least 1");
    CMT_REQUIRE(a->ncls >= 1, "cmt_track_predict: ncls must be at least 1");
    CMT_REQUIRE_SUPPORTED(a->T <= CMT_TRACK_MAX_TRACKS, "cmt_track_predict: T above 512 is not supported");
    CMT_REQUIRE_SUPPORTED(a->D <= CMT_TRACK_MAX_DETS, "cmt_track_predict: D above 1024 is not supported");
    CMT_REQUIRE_SUPPORTED(a->ncls <= CMT_TRACK_MAX_CLASSES, "cmt_track_predict: ncls above 32 is not supported");
    CMT_REQUIRE(a->ld >= 9, "cmt_track_predict: ld must be at least 9");
    CMT_REQUIRE(trk_nonneg(a->dt), "cmt_track_predict: dt must be finite and not negative");
    CMT_REQUIRE(trk_nonneg(a->q_pos) && trk_nonneg(a->q_vel), "cmt_track_predict: q_pos and q_vel must be finite and not negative");
    CMT_REQUIRE(!std::isnan(a->score_thr), "cmt_track_predict: score_thr must not be NaN");
    if (a->has_pose) {
        bool fin = std::isfinite(a->pose_yaw);
        for (int k = 0; k < 12; ++k) fin = fin && std::isfinite(a->pose[k]);
        CMT_REQUIRE(fin, "cmt_track_predict: pose and pose_yaw must be finite");
    }
    CMT_REQUIRE(ptr_aligned(a->trk_f, 4) && ptr_aligned(a->trk_i, 4), "cmt_track_predict: the state (trk_f, trk_i) must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->det, 4) && ptr_aligned(a->scores, 4) && ptr_aligned(a->labels, 4) && ptr_aligned(a->gate2, 4),
                "cmt_track_predict: det, scores, labels and gate2 must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->count, 4), "cmt_track_predict: count must be 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->det_w, 4) && ptr_aligned(a->det_ok, 4) && ptr_aligned(a->live, 4) && ptr_aligned(a->cost, 4) && ptr_aligned(a->lsap_desc, 8),
                "cmt_track_predict: det_w, det_ok, live, cost (4 bytes) and lsap_desc (8 bytes) must be non-null and aligned");
    trp_p p;
    p.trk_f = (float*)a->trk_f, p.trk_i = a->trk_i;
    p.det = (const float*)a->det, p.scores = (const float*)a->scores, p.labels = a->labels, p.count = a->count;
    p.gate2 = (const float*)a->gate2;
    p.det_w = (float*)a->det_w, p.det_ok = a->det_ok, p.live = a->live, p.cost = (float*)a->cost;
    p.desc = (long long*)a->lsap_desc;
    p.T = a->T, p.D = a->D, p.ld = a->ld, p.ncls = a->ncls, p.has_pose = a->has_pose ? 1 : 0;
    p.dt = a->dt, p.q_pos = a->q_pos, p.q_vel = a->q_vel, p.score_thr = a->score_thr, p.pose_yaw = a->pose_yaw;
    for (int k = 0; k < 12; ++k) p.m[k] = a->pose[k];
    const hipStream_t st = (hipStream_t)stream;
    track_predict_kernel<<<dim3(1), TRK_THREADS, 0, st>>>(p);
    track_cost_kernel<<<dim3((unsigned)cdiv64(a->D, TRK_THREADS), (unsigned)cdiv64(a->T, TRK_ROWS)), TRK_THREADS, 0, st>>>(p);
    return cmt_check_launch("cmt_track_predict");
}

extern "C" int cmt_track_update(const cmt_track_update_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_track_update: null argument struct");
    CMT_REQUIRE(a->T >= 1 && a->D >= 1, "cmt_track_update: T and D must be at least 1");
    CMT_REQUIRE(a->H >= 1, "cmt_track_update: H must be at least 1");
    CMT_REQUIRE_SUPPORTED(a->T <= CMT_TRACK_MAX_TRACKS, "cmt_track_update: T above 512 is not supported");
    CMT_REQUIRE_SUPPORTED(a->D <= CMT_TRACK_MAX_DETS, "cmt_track_update: D above 1024 is not supported");
    CMT_REQUIRE_SUPPORTED(a->H <= CMT_TRACK_MAX_HISTORY, "cmt_track_update: H above 32 is not supported");
    CMT_REQUIRE(a->max_age >= 0, "cmt_track_update: max_age must not be negative");
    CMT_REQUIRE(trk_pos(a->r_pos) && trk_pos(a->r_vel), "cmt_track_update: r_pos and r_vel must be finite and positive");
    CMT_REQUIRE(trk_nonneg(a->p0_pos) && trk_nonneg(a->p0_vel), "cmt_track_update: p0_pos and p0_vel must be finite and not negative");
    CMT_REQUIRE(!std::isnan(a->birth_thr), "cmt_track_update: birth_thr must not be NaN");
    CMT_REQUIRE(ptr_aligned(a->trk_f, 4) && ptr_aligned(a->trk_i, 4) && ptr_aligned(a->hist, 4) && ptr_aligned(a->counters, 4),
                "cmt_track_update: the state (trk_f, trk_i, hist, counters) must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->live, 4) && ptr_aligned(a->lsap_desc, 8) && ptr_aligned(a->cost, 4) && ptr_aligned(a->match_g, 4) && ptr_aligned(a->match_q, 4),
                "cmt_track_update: live, cost, match_g, match_q (4 bytes) and lsap_desc (8 bytes) must be non-null and aligned");
    CMT_REQUIRE(ptr_aligned(a->det_w, 4) && ptr_aligned(a->scores, 4) && ptr_aligned(a->labels, 4) && ptr_aligned(a->det_ok, 4),
                "cmt_track_update: det_w, scores, labels and det_ok must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->det_track, 4) && ptr_aligned(a->det_slot, 4), "cmt_track_update: det_track and det_slot must be non-null and 4-byte aligned");
    tru_p p;
    p.trk_f = (float*)a->trk_f, p.trk_i = a->trk_i, p.hist = (float*)a->hist, p.counters = a->counters;
    p.live = a->live, p.desc = (const long long*)a->lsap_desc, p.cost = (const float*)a->cost;
    p.match_g = a->match_g, p.match_q = a->match_q;
    p.det_w = (const float*)a->det_w, p.scores = (const float*)a->scores, p.labels = a->labels, p.det_ok = a->det_ok;
    p.det_track = a->det_track, p.det_slot = a->det_slot;
    p.T = a->T, p.D = a->D, p.H = a->H, p.use_velocity = a->use_velocity ? 1 : 0, p.max_age = a->max_age;
    p.r_pos = a->r_pos, p.r_vel = a->r_vel, p.p0_pos = a->p0_pos, p.p0_vel = a->p0_vel, p.birth_thr = a->birth_thr;
    track_update_kernel<<<dim3(1), TRK_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_track_update");
}
