// Tracking evaluation on the device: CLEAR MOT counters per recall level and their AMOTA / AMOTP summary, the
// contract of include/cmt_hip.h (cmt_mot_eval_*).  No contraction anywhere in this file (see the Makefile): the
// float32 distances and the float64 metrics are single IEEE operations, each rounded on its own.
//
//   mot_keys_kernel        one thread per row: the filters and the int64 sort key (frame position, class, row).  The
//                          caller sorts the keys; a (frame, class) is then one contiguous run in row order.
//   mot_runs_kernel        C workgroups count npos, 2 x 64 more find the longest run that ends in their share of each
//                          side (a binary search at every run end): the caller sizes the matrices from their maxima.
//   mot_cost_kernel        one WAVE per chain and step, four chains in a workgroup, no barrier: a chain's frame has a
//                          handful of boxes (the caps are 512 x 2048), so a chain is latency, and tens of thousands
//                          of chains fill the device.  track.hip needs ONE workgroup because its total orders span
//                          1024 entries with LDS tables; here every order is inside one wave: the active predictions
//                          are compacted in row order by ballot + wave_rank (wave_ops.h) over chunks of 64, the
//                          sticky pass walks the ground truth that has a previous track (a ballot's set bits, in
//                          order) and finds the lowest matching column by a ballot over the column chunks.  Taken
//                          bits live in registers: lane l owns columns l, l + 64, ... (32 bits) and rows l, l + 64, ...
//                          (8 bits); a row's bit reaches the other lanes by a shuffle.  The compacted column list is
//                          written to memory by one lane and read by another of the same wave: a workgroup fence
//                          stands between.
//   (cmt_lsap)             one wave per chain, unchanged.
//   mot_update_kernel      one wave per chain: lane l accounts row base + l; the counters are ballot population
//                          counts, the distance sum walks the matched lanes in order (a shuffle per term).
//   mot_thresholds_kernel  one workgroup per class, thread k = slot k: an order statistic of the sorted scores.
//   mot_summary_kernel     one workgroup per class, thread k = slot k sums its chains over the scenes in order, then
//                          thread 0 walks the slots.
#include "wave_ops.h"

#include <cmath>
#include <cstdint>

constexpr int MOT_THREADS = 256;
constexpr int MOT_WAVES = MOT_THREADS / 64;
constexpr int64_t MOT_NONE = INT64_MAX;
constexpr int64_t MOT_ROW_MASK = 0xffffffffll;
static_assert(CMT_MOT_MAX_PRED / 64 <= 32 && CMT_MOT_MAX_GT / 64 <= 32, "a lane's taken bits fit one word");

typedef cmt_mot_eval_args mot_p;

__device__ __forceinline__ double mot_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ int64_t mot_lower_bound(const int64_t* k, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (k[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the float32 centre distance of the contract
__device__ __forceinline__ float mot_dist(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    const float xx = dx * dx, yy = dy * dy;
    return sqrtf(xx + yy);
}

// (scene * Fmax + step) << 6 | class of a row, or -1: the frame table, the label and the range test
__device__ __forceinline__ int64_t mot_row_key(const mot_p& p, int c, int f, float xf, float yf) {
    if (c < 0 || c >= p.C || f < 0 || f >= p.F) return -1;
    const int* tab = (const int*)p.frame_tab + 2 * (int64_t)f;
    const int scene = tab[0], step = tab[1];
    if (scene < 0 || scene >= p.S || step < 0 || step >= p.Fmax) return -1;
    if (!finite32(xf) || !finite32(yf)) return -1;
    const double x = (double)xf, y = (double)yf;
    const double xx = x * x, yy = y * y;
    if (!(sqrt(xx + yy) < p.range[c])) return -1;
    return (((int64_t)scene * p.Fmax + step) << 6) | (int64_t)c;
}

__global__ __launch_bounds__(MOT_THREADS) void mot_keys_kernel(mot_p p) {
    const int64_t i = (int64_t)blockIdx.x * MOT_THREADS + threadIdx.x;
    if (i < p.N) {
        int64_t k = MOT_NONE;
        if (i < clamp_count(p.n_pred, p.N)) {
            const float* b = (const float*)p.pred_box + i * p.ld_pred;
            const int64_t fk = mot_row_key(p, ((const int*)p.pred_label)[i], ((const int*)p.pred_frame)[i], b[0], b[1]);
            if (fk >= 0 && ((const int*)p.pred_track)[i] >= 0 && finite32(((const float*)p.pred_score)[i])) k = (fk << 32) | i;
        }
        ((int64_t*)p.key_pred)[i] = k;
    }
    if (i < p.G) {
        int64_t k = MOT_NONE;
        if (i < clamp_count(p.n_gt, p.G)) {
            const float* b = (const float*)p.gt_box + i * p.ld_gt;
            const int64_t fk = mot_row_key(p, ((const int*)p.gt_label)[i], ((const int*)p.gt_frame)[i], b[0], b[1]);
            const int o = ((const int*)p.gt_inst)[i];
            if (fk >= 0 && o >= 0 && o < p.max_gt_tracks) k = (fk << 32) | i;
        }
        ((int64_t*)p.key_gt)[i] = k;
        if (k == MOT_NONE) {   // a kept row gets both from phase 1's update
            ((unsigned*)p.tp_score)[i] = QNAN32;
            ((int64_t*)p.tp_key)[i] = MOT_NONE;
        }
    }
}

// the longest run of equal (frame, class) that ends in this workgroup's share of the sorted keys (workgroup `slice` of
// CMT_MOT_RUN_PARTS takes every CMT_MOT_RUN_PARTS-th tile of 256 keys)
__device__ __forceinline__ int mot_longest_run(const int64_t* sk, int64_t n, int slice, int* part) {
    int best = 0;
    for (int64_t j = (int64_t)slice * MOT_THREADS + threadIdx.x; j < n; j += (int64_t)CMT_MOT_RUN_PARTS * MOT_THREADS) {
        const int64_t k = sk[j];
        if (k == MOT_NONE) continue;
        const int64_t fk = k >> 32;
        if (j + 1 < n && (sk[j + 1] >> 32) == fk) continue;   // not the run's end (INT64_MAX >> 32 is above every fk)
        const int64_t len = j + 1 - mot_lower_bound(sk, n, fk << 32);
        best = len > best ? (int)len : best;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MOT_WAVES; ++w) best = part[w] > best ? part[w] : best;
    return best;
}

__global__ __launch_bounds__(MOT_THREADS) void mot_runs_kernel(mot_p p) {
    __shared__ int part[MOT_WAVES];
    const int x = (int)blockIdx.x;
    const int64_t* skg = (const int64_t*)p.sk_gt;
    if (x < p.C) {
        int n = 0;
        for (int64_t j = threadIdx.x; j < p.G; j += MOT_THREADS) {
            const int64_t k = skg[j];
            n += (k != MOT_NONE && (int)((k >> 32) & 63) == x) ? 1 : 0;
        }
        n = wave_sum(n);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
        __syncthreads();
        if (threadIdx.x == 0) ((int*)p.npos)[x] = part[0] + part[1] + part[2] + part[3];
    } else {
        const bool gt = x - p.C < CMT_MOT_RUN_PARTS;
        const int slice = (x - p.C) % CMT_MOT_RUN_PARTS;
        const int r = mot_longest_run(gt ? skg : (const int64_t*)p.sk_pred, gt ? p.G : p.N, slice, part);
        if (threadIdx.x == 0) ((int*)p.run_max)[(gt ? 0 : CMT_MOT_RUN_PARTS) + slice] = r;
    }
}

// ---- one chain, one step ------------------------------------------------------------------------------------

struct mot_chain {
    int local, c;        // the chain's place in the block, its class
    int64_t number, fk;  // its number in the phase, the (frame, class) key of this step
    float thr, dist_th;
    bool all_active, runs;   // phase 1; the slot is achieved
};

__device__ __forceinline__ bool mot_chain_of(const mot_p& p, mot_chain& ch) {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    ch.local = (int)blockIdx.x * MOT_WAVES + w;
    if (ch.local >= p.nchains) return false;
    ch.number = (int64_t)p.chain0 + ch.local;
    int64_t sc = ch.number;
    ch.all_active = p.phase == 1;
    ch.thr = 0.f;
    ch.runs = true;
    if (!ch.all_active) {
        const int k = (int)(sc % p.R);
        sc /= p.R;
        ch.thr = ((const float*)p.thr)[(sc % p.C) * p.R + k];
        ch.runs = ch.thr == ch.thr;
    }
    ch.c = (int)(sc % p.C);
    ch.fk = (((sc / p.C) * p.Fmax + p.step) << 6) | (int64_t)ch.c;
    ch.dist_th = p.dist_th[ch.c];
    return true;
}

__global__ __launch_bounds__(MOT_THREADS) void mot_cost_kernel(mot_p p) {
    mot_chain ch;
    if (!mot_chain_of(p, ch)) return;
    const int lane = (int)threadIdx.x & 63;
    const int64_t* skg = (const int64_t*)p.sk_gt;
    const int64_t* skp = (const int64_t*)p.sk_pred;
    const float* pbox = (const float*)p.pred_box;
    const float* gbox = (const float*)p.gt_box;
    const int* ptrack = (const int*)p.pred_track;
    int* state_m = (int*)p.state_m + (int64_t)ch.local * p.max_gt_tracks;
    int64_t* desc = (int64_t*)p.desc + 4 * (int64_t)ch.local;
    const int64_t off = (int64_t)ch.local * p.Gmax * p.Hmax;

    if (p.step == 0) {   // the state's first writer; this launch does not read it at step 0
        unsigned char* lost = (unsigned char*)p.state_lost + (int64_t)ch.local * p.max_gt_tracks;
        for (int o = lane; o < p.max_gt_tracks; o += 64) state_m[o] = -1, lost[o] = 0;
    }
    int ng = 0, nrun = 0;
    int64_t g0 = 0, p0 = 0;
    if (ch.runs) {
        g0 = mot_lower_bound(skg, p.G, ch.fk << 32);
        p0 = mot_lower_bound(skp, p.N, ch.fk << 32);
        const int64_t gl = mot_lower_bound(skg, p.G, (ch.fk + 1) << 32) - g0, pl = mot_lower_bound(skp, p.N, (ch.fk + 1) << 32) - p0;
        ng = (int)(gl < p.Gmax ? gl : p.Gmax);
        nrun = (int)(pl < p.Hmax ? pl : p.Hmax);
    }
    // the active predictions, compacted in row order
    int* cols = (int*)p.cols + (int64_t)ch.local * p.Hmax;
    int na = 0;
    for (int base = 0; base < nrun; base += 64) {
        const int q = base + lane;
        int row = 0;
        bool act = false;
        if (q < nrun) {
            row = (int)(skp[p0 + q] & MOT_ROW_MASK);
            act = ch.all_active || ((const float*)p.pred_score)[row] >= ch.thr;
        }
        const unsigned long long m = __ballot(act);
        if (act) cols[na + wave_rank(m)] = row;
        na += __popcll(m);
    }
    if (lane == 0) desc[0] = off, desc[1] = ng, desc[2] = na, desc[3] = p.Hmax;
    if (ng == 0) return;
    int* smatch = (int*)p.smatch + (int64_t)ch.local * p.Gmax;
    __threadfence_block();   // cols: written by one lane, read by another of this wave

    // the sticky pass
    unsigned ctaken = 0, rtaken = 0;   // bit k: column k * 64 + lane, row k * 64 + lane
    for (int base = 0; base < ng; base += 64) {
        const int i = base + lane;
        int mi = -1;
        float gx = 0.f, gy = 0.f;
        if (i < ng) {
            const int64_t grow = skg[g0 + i] & MOT_ROW_MASK;
            gx = gbox[grow * p.ld_gt], gy = gbox[grow * p.ld_gt + 1];
            if (p.step > 0) mi = state_m[clamp_index(((const int*)p.gt_inst)[grow], p.max_gt_tracks - 1)];
        }
        int mine = -1;
        unsigned long long todo = __ballot(mi >= 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int want = __shfl(mi, l, 64);
            const float x = __shfl(gx, l, 64), y = __shfl(gy, l, 64);
            int found = -1;
            for (int kc = 0; kc * 64 < na && found < 0; ++kc) {
                const int j = kc * 64 + lane;
                bool cand = false;
                if (j < na && !((ctaken >> kc) & 1u)) {
                    const int row = cols[j];
                    if (ptrack[row] == want) cand = mot_dist(x, y, pbox[(int64_t)row * p.ld_pred], pbox[(int64_t)row * p.ld_pred + 1]) < ch.dist_th;
                }
                const unsigned long long hit = __ballot(cand);
                if (hit) {
                    const int hl = __ffsll((long long)hit) - 1;
                    found = kc * 64 + hl;
                    if (lane == hl) ctaken |= 1u << kc;
                }
            }
            if (lane == l) mine = found;
        }
        if (mine >= 0) rtaken |= 1u << (base >> 6);
        if (i < ng) smatch[i] = mine;
    }

    // the cost matrix: a lane owns a column, the rows are the same in every lane
    float* cost = (float*)p.cost + off;
    for (int kc = 0; kc * 64 < na; ++kc) {
        const int j = kc * 64 + lane;
        const bool have = j < na;
        const int row = have ? cols[j] : 0;
        const float px = have ? pbox[(int64_t)row * p.ld_pred] : 0.f, py = have ? pbox[(int64_t)row * p.ld_pred + 1] : 0.f;
        const bool cfree = have && !((ctaken >> kc) & 1u);
        for (int i = 0; i < ng; ++i) {
            const int64_t grow = skg[g0 + i] & MOT_ROW_MASK;
            const bool rfree = !((__shfl(rtaken, i & 63, 64) >> (i >> 6)) & 1u);
            const float d = mot_dist(gbox[grow * p.ld_gt], gbox[grow * p.ld_gt + 1], px, py);
            if (have) cost[(int64_t)i * p.Hmax + j] = (cfree && rfree && d < ch.dist_th) ? d : CMT_MOT_BIG;
        }
    }
}

__global__ __launch_bounds__(MOT_THREADS) void mot_update_kernel(mot_p p) {
    mot_chain ch;
    if (!mot_chain_of(p, ch)) return;
    const int lane = (int)threadIdx.x & 63;
    const int64_t* skg = (const int64_t*)p.sk_gt;
    const float* pbox = (const float*)p.pred_box;
    const float* gbox = (const float*)p.gt_box;
    const int64_t* desc = (const int64_t*)p.desc + 4 * (int64_t)ch.local;
    const int ng = clamp_index(desc[1], p.Gmax), na = clamp_index(desc[2], p.Hmax);
    const int64_t off = (int64_t)ch.local * p.Gmax * p.Hmax;
    int64_t* cnt = (int64_t*)(p.phase == 1 ? p.chain_cnt1 : p.chain_cnt2) + 6 * ch.number;
    double* dsum = (double*)(p.phase == 1 ? p.chain_dist1 : p.chain_dist2) + ch.number;
    int64_t n[6] = {0, 0, 0, 0, 0, 0};
    double dist = 0.0;
    if (p.step > 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) n[k] = cnt[k];
        dist = *dsum;
    }
    if (ng > 0) {
        const int64_t g0 = mot_lower_bound(skg, p.G, ch.fk << 32);
        const int* cols = (const int*)p.cols + (int64_t)ch.local * p.Hmax;
        const int* smatch = (const int*)p.smatch + (int64_t)ch.local * p.Gmax;
        const int* mg = p.match_g + (int64_t)ch.local * p.Gmax;
        const int* mq = p.match_q + (int64_t)ch.local * p.Hmax;
        const float* cost = (const float*)p.cost + off;
        int* state_m = (int*)p.state_m + (int64_t)ch.local * p.max_gt_tracks;
        unsigned char* state_lost = (unsigned char*)p.state_lost + (int64_t)ch.local * p.max_gt_tracks;
        int tp = 0;
        for (int base = 0; base < ng; base += 64) {
            const int i = base + lane;
            const bool ok = i < ng;
            bool matched = false, ids = false, frag = false;
            float d = 0.f;
            if (ok) {
                const int64_t grow = skg[g0 + i] & MOT_ROW_MASK;   // below G: a sorted key of a kept row
                const int o = clamp_index(((const int*)p.gt_inst)[grow], p.max_gt_tracks - 1);
                int j = smatch[i];
                if (j >= 0 && j < na) {   // the sticky pass: the same distance again
                    const int64_t prow = cols[j];
                    d = mot_dist(gbox[grow * p.ld_gt], gbox[grow * p.ld_gt + 1], pbox[prow * p.ld_pred], pbox[prow * p.ld_pred + 1]);
                    matched = true;
                } else {
                    j = mg[i];
                    if (j >= 0 && j < na && mq[j] == i) {
                        d = cost[(int64_t)i * p.Hmax + j];
                        matched = d < CMT_MOT_BIG;
                    }
                }
                const int mo = state_m[o];
                if (matched) {
                    const int64_t prow = cols[j];
                    const int h = ((const int*)p.pred_track)[prow];
                    ids = mo >= 0 && mo != h;
                    frag = state_lost[o] != 0;
                    state_m[o] = h, state_lost[o] = 0;
                } else {
                    state_lost[o] = mo >= 0 ? 1 : 0;
                }
                if (p.phase == 1) {
                    const float s = matched ? ((const float*)p.pred_score)[cols[j]] : __uint_as_float(QNAN32);
                    ((float*)p.tp_score)[grow] = s;
                    ((int64_t*)p.tp_key)[grow] = matched ? (((int64_t)ch.c << 32) | (int64_t)score_desc_key(s)) : MOT_NONE;
                }
            }
            unsigned long long hit = __ballot(matched);
            tp += __popcll(hit);
            n[3] += __popcll(__ballot(ids));
            n[4] += __popcll(__ballot(frag));
            while (hit) {   // the distances in row order
                const int l = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                dist = dist + (double)__shfl(d, l, 64);
            }
        }
        n[0] += tp;
        n[2] += ng - tp;
        n[1] += na - tp;
    } else {
        n[1] += na;
    }
    n[5] += na;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) cnt[k] = n[k];
        *dsum = dist;
    }
}

__global__ __launch_bounds__(64) void mot_thresholds_kernel(mot_p p) {
    const int c = (int)blockIdx.x, k = (int)threadIdx.x;
    if (k >= p.R) return;
    const int64_t* sk = (const int64_t*)p.sk_tp;
    const int64_t a = mot_lower_bound(sk, p.G, (int64_t)c << 32);
    const int64_t ntp = mot_lower_bound(sk, p.G, (int64_t)(c + 1) << 32) - a;
    const int npos = ((const int*)p.npos)[c];
    const double want = ceil(p.recall[k] * (double)npos);
    int64_t need = (int64_t)want;
    need = need < 1 ? 1 : need;
    float t = __uint_as_float(QNAN32);
    if (npos > 0 && need <= ntp) {
        const int64_t g = ((const int64_t*)p.si_tp)[a + need - 1];
        if (g >= 0 && g < p.G) t = ((const float*)p.tp_score)[g];
    }
    ((float*)p.thr)[c * p.R + k] = t;
}

__global__ __launch_bounds__(64) void mot_summary_kernel(mot_p p) {
    __shared__ double s_metric[CMT_MOT_MAX_THRESHOLDS][4];
    __shared__ int64_t s_cnt[CMT_MOT_MAX_THRESHOLDS][6];
    __shared__ int s_ok[CMT_MOT_MAX_THRESHOLDS];
    const int c = (int)blockIdx.x, k = (int)threadIdx.x;
    const int npos = ((const int*)p.npos)[c];
    const double dn = (double)npos, th = (double)p.dist_th[c];
    if (k < p.R) {
        int64_t n[6] = {0, 0, 0, 0, 0, 0};
        double dist = 0.0;
        for (int s = 0; s < p.S; ++s) {
            const int64_t chain = ((int64_t)s * p.C + c) * p.R + k;
            const int64_t* q = (const int64_t*)p.chain_cnt2 + 6 * chain;
#pragma unroll
            for (int e = 0; e < 6; ++e) n[e] += q[e];
            dist = dist + ((const double*)p.chain_dist2)[chain];
        }
        const float t = ((const float*)p.thr)[c * p.R + k];
        const bool ok = t == t;
        double m[4] = {0.0, 0.0, th, 0.0};   // recall, MOTA, MOTP, MOTAR of a slot not achieved
        if (npos == 0) {
            m[0] = m[1] = m[2] = m[3] = mot_nan();
        } else if (ok) {
            const double e = (double)(n[3] + n[1] + n[2]), tp = (double)n[0];
            m[0] = tp / dn;
            m[1] = 1.0 - e / dn;
            if (n[0] > 0) {
                m[2] = dist / tp;
                const double miss = (1.0 - m[0]) * dn, den = m[0] * dn;
                const double v = 1.0 - (e - miss) / den;
                m[3] = v > 0.0 ? v : 0.0;
            }
        }
        int64_t* oc = (int64_t*)p.counters + ((int64_t)c * p.R + k) * 6;
        double* om = (double*)p.metrics + ((int64_t)c * p.R + k) * 4;
#pragma unroll
        for (int e = 0; e < 6; ++e) oc[e] = n[e], s_cnt[k][e] = n[e];
#pragma unroll
        for (int e = 0; e < 4; ++e) om[e] = m[e], s_metric[k][e] = m[e];
        ((double*)p.dist_sum)[c * p.R + k] = dist;
        s_ok[k] = ok && npos > 0 ? 1 : 0;
    }
    __syncthreads();
    if (k == 0) {
        double* o = (double*)p.class_sum + (int64_t)c * 12;
        double sa = 0.0, sp = 0.0;
        int best = -1;
        for (int r = 0; r < p.R; ++r) {
            sa = sa + s_metric[r][3];
            sp = sp + s_metric[r][2];
            if (s_ok[r] && (best < 0 || s_metric[r][1] > s_metric[best][1])) best = r;
        }
        for (int e = 0; e < 12; ++e) o[e] = mot_nan();
        if (npos > 0) o[0] = sa / (double)p.R, o[1] = sp / (double)p.R;
        o[2] = (double)best;
        if (best >= 0) {
            o[3] = s_metric[best][1], o[4] = s_metric[best][2], o[5] = s_metric[best][0];
            o[6] = (double)s_cnt[best][0], o[7] = (double)s_cnt[best][1], o[8] = (double)s_cnt[best][2];
            o[9] = (double)s_cnt[best][3], o[10] = (double)s_cnt[best][4];
            o[11] = (double)((const float*)p.thr)[c * p.R + best];
        }
    } else if (k == 1) {   // the block has 64 threads whatever R is
        int64_t n[6] = {0, 0, 0, 0, 0, 0};
        double dist = 0.0;
        for (int s = 0; s < p.S; ++s) {
            const int64_t chain = (int64_t)s * p.C + c;
            const int64_t* q = (const int64_t*)p.chain_cnt1 + 6 * chain;
#pragma unroll
            for (int e = 0; e < 6; ++e) n[e] += q[e];
            dist = dist + ((const double*)p.chain_dist1)[chain];
        }
        int64_t* oc = (int64_t*)p.counters1 + (int64_t)c * 6;
#pragma unroll
        for (int e = 0; e < 6; ++e) oc[e] = n[e];
        ((double*)p.dist_sum1)[c] = dist;
    }
}

// ---- entry points -------------------------------------------------------------------------------------------

extern "C" int64_t cmt_mot_eval_args_size(void) { return (int64_t)sizeof(cmt_mot_eval_args); }

static int mot_check_base(const cmt_mot_eval_args* a, const char* who) {
    const std::string w(who);
    CMT_REQUIRE(a != nullptr, w + ": null argument struct");
    CMT_REQUIRE(a->N >= 0 && a->N < ((int64_t)1 << 31), w + ": N must be in [0, 2^31)");
    CMT_REQUIRE(a->G >= 0 && a->G < ((int64_t)1 << 31), w + ": G must be in [0, 2^31)");
    CMT_REQUIRE(a->F >= 1 && a->S >= 1 && a->Fmax >= 1, w + ": F, S and Fmax must be at least 1");
    CMT_REQUIRE((int64_t)a->S * a->Fmax <= ((int64_t)1 << 24), w + ": S * Fmax must be at most 2^24");
    CMT_REQUIRE(a->C >= 1 && a->R >= 1, w + ": C and R must be at least 1");
    CMT_REQUIRE(a->max_gt_tracks >= 1, w + ": max_gt_tracks must be at least 1");
    CMT_REQUIRE_SUPPORTED(a->C <= CMT_MOT_MAX_CLASSES, w + ": C above 64 is not supported");
    CMT_REQUIRE_SUPPORTED(a->R <= CMT_MOT_MAX_THRESHOLDS, w + ": R above 64 is not supported");
    CMT_REQUIRE_SUPPORTED(a->max_gt_tracks <= CMT_MOT_MAX_GT_TRACKS, w + ": max_gt_tracks above 65536 is not supported");
    CMT_REQUIRE(a->ld_pred >= 2 && a->ld_gt >= 2, w + ": ld_pred and ld_gt must be at least 2");
    for (int c = 0; c < a->C; ++c) {
        CMT_REQUIRE(std::isfinite(a->range[c]) && a->range[c] > 0.0, w + ": range must be finite and positive");
        CMT_REQUIRE(std::isfinite(a->dist_th[c]) && a->dist_th[c] > 0.f, w + ": dist_th must be finite and positive");
    }
    for (int k = 0; k < a->R; ++k)
        CMT_REQUIRE(a->recall[k] > 0.0 && a->recall[k] <= 1.0, w + ": recall levels must be in (0, 1]");
    return 0;
}

#define MOT_PTR(field, al, rows)                                                                                     \
    CMT_REQUIRE((rows) == 0 || ptr_aligned(a->field, al), std::string(who) + ": " #field " must be non-null and " #al \
                                                                                 "-byte aligned")

static int mot_check_rows(const cmt_mot_eval_args* a, const char* who) {
    MOT_PTR(pred_box, 4, a->N); MOT_PTR(pred_score, 4, a->N); MOT_PTR(pred_label, 4, a->N); MOT_PTR(pred_track, 4, a->N);
    MOT_PTR(pred_frame, 4, a->N);
    MOT_PTR(gt_box, 4, a->G); MOT_PTR(gt_label, 4, a->G); MOT_PTR(gt_frame, 4, a->G); MOT_PTR(gt_inst, 4, a->G);
    MOT_PTR(tp_score, 4, a->G); MOT_PTR(tp_key, 8, a->G);
    return 0;
}

static int mot_check_step(const cmt_mot_eval_args* a, const char* who) {
    const std::string w(who);
    if (int rc = mot_check_base(a, who)) return rc;
    CMT_REQUIRE(a->phase == 1 || a->phase == 2, w + ": phase must be 1 or 2");
    CMT_REQUIRE(a->step >= 0 && a->step < a->Fmax, w + ": step must be in [0, Fmax)");
    const int64_t chains = (int64_t)a->S * a->C * (a->phase == 2 ? a->R : 1);
    CMT_REQUIRE(a->chain0 >= 0 && a->nchains >= 1 && (int64_t)a->chain0 + a->nchains <= chains,
                w + ": chain0, nchains must name chains of the phase");
    CMT_REQUIRE(a->Gmax >= 0 && a->Hmax >= 0, w + ": Gmax and Hmax must not be negative");
    CMT_REQUIRE_SUPPORTED(a->nchains <= CMT_MOT_MAX_CHAINS, w + ": more than 65535 chains per call are not supported");
    CMT_REQUIRE_SUPPORTED(a->Gmax <= CMT_MOT_MAX_GT, w + ": more than 512 ground-truth boxes per (frame, class) are not supported");
    CMT_REQUIRE_SUPPORTED(a->Hmax <= CMT_MOT_MAX_PRED, w + ": more than 2048 predictions per (frame, class) are not supported");
    if (int rc = mot_check_rows(a, who)) return rc;
    MOT_PTR(sk_pred, 8, a->N); MOT_PTR(sk_gt, 8, a->G);
    MOT_PTR(state_m, 4, 1); MOT_PTR(state_lost, 1, 1); MOT_PTR(desc, 8, 1);
    MOT_PTR(cost, 4, a->Gmax * a->Hmax); MOT_PTR(cols, 4, a->Hmax); MOT_PTR(smatch, 4, a->Gmax);
    if (a->phase == 2) MOT_PTR(thr, 4, 1);
    return 0;
}

extern "C" int cmt_mot_eval_keys(const cmt_mot_eval_args* a, void* stream) {
    const char* who = "cmt_mot_eval_keys";
    if (int rc = mot_check_base(a, who)) return rc;
    if (int rc = mot_check_rows(a, who)) return rc;
    CMT_REQUIRE(ptr_aligned_or_null(a->n_pred, 4) && ptr_aligned_or_null(a->n_gt, 4),
                std::string(who) + ": n_pred and n_gt must be 4-byte aligned");
    MOT_PTR(frame_tab, 4, 1); MOT_PTR(key_pred, 8, a->N); MOT_PTR(key_gt, 8, a->G);
    const int64_t rows = a->N > a->G ? a->N : a->G;
    if (rows > 0) mot_keys_kernel<<<dim3((unsigned)cdiv64(rows, MOT_THREADS)), MOT_THREADS, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(who);
}

extern "C" int cmt_mot_eval_runs(const cmt_mot_eval_args* a, void* stream) {
    const char* who = "cmt_mot_eval_runs";
    if (int rc = mot_check_base(a, who)) return rc;
    MOT_PTR(sk_pred, 8, a->N); MOT_PTR(sk_gt, 8, a->G); MOT_PTR(npos, 4, 1); MOT_PTR(run_max, 4, 1);
    mot_runs_kernel<<<dim3((unsigned)(a->C + 2 * CMT_MOT_RUN_PARTS)), MOT_THREADS, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(who);
}

extern "C" int cmt_mot_eval_cost(const cmt_mot_eval_args* a, void* stream) {
    const char* who = "cmt_mot_eval_cost";
    if (int rc = mot_check_step(a, who)) return rc;
    mot_cost_kernel<<<dim3((unsigned)cdiv64(a->nchains, MOT_WAVES)), MOT_THREADS, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(who);
}

extern "C" int cmt_mot_eval_update(const cmt_mot_eval_args* a, void* stream) {
    const char* who = "cmt_mot_eval_update";
    if (int rc = mot_check_step(a, who)) return rc;
    MOT_PTR(match_q, 4, a->Hmax); MOT_PTR(match_g, 4, a->Gmax);
    if (a->phase == 1) { MOT_PTR(chain_cnt1, 8, 1); MOT_PTR(chain_dist1, 8, 1); }
    else { MOT_PTR(chain_cnt2, 8, 1); MOT_PTR(chain_dist2, 8, 1); }
    mot_update_kernel<<<dim3((unsigned)cdiv64(a->nchains, MOT_WAVES)), MOT_THREADS, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(who);
}

extern "C" int cmt_mot_eval_thresholds(const cmt_mot_eval_args* a, void* stream) {
    const char* who = "cmt_mot_eval_thresholds";
    if (int rc = mot_check_base(a, who)) return rc;
    MOT_PTR(sk_tp, 8, a->G); MOT_PTR(si_tp, 8, a->G); MOT_PTR(tp_score, 4, a->G); MOT_PTR(npos, 4, 1); MOT_PTR(thr, 4, 1);
    mot_thresholds_kernel<<<dim3((unsigned)a->C), 64, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(who);
}

extern "C" int cmt_mot_eval_summary(const cmt_mot_eval_args* a, void* stream) {
    const char* who = "cmt_mot_eval_summary";
    if (int rc = mot_check_base(a, who)) return rc;
    MOT_PTR(npos, 4, 1); MOT_PTR(thr, 4, 1);
    MOT_PTR(chain_cnt1, 8, 1); MOT_PTR(chain_dist1, 8, 1); MOT_PTR(chain_cnt2, 8, 1); MOT_PTR(chain_dist2, 8, 1);
    MOT_PTR(counters, 8, 1); MOT_PTR(dist_sum, 8, 1); MOT_PTR(metrics, 8, 1); MOT_PTR(class_sum, 8, 1);
    MOT_PTR(counters1, 8, 1); MOT_PTR(dist_sum1, 8, 1);
    mot_summary_kernel<<<dim3((unsigned)a->C), 64, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(who);
}
