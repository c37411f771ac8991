// mot_eval.hip — multi-object-tracking evaluation (TrackEval's HOTA, CLEAR and Identity for MotChallenge2DBox on the data the reference's
// writer produces) on the device.  The rule is stated in include/centernet_gfx950.h and restated in numpy + scipy in
// tests/mot_eval_ref.py; every float64 operation is rounded on its own and every sum runs in the stated order, so the two agree bit
// for bit.  The assignment is lsap_device.h's, which reproduces scipy.optimize.linear_sum_assignment, ties included.
//
// All sequences of an evaluation share every launch.  The input is pooled: frame f of the evaluation owns ground truths
// gt_off[f] .. gt_off[f + 1], predictions pr_off[f] .. and the ng x np matrix at sim_off[f]; sequence s owns frames seq_frm[s] ..,
// ground-truth ids seq_gid[s] .., tracker ids seq_tid[s] .. and the G x T pair block at seq_pair[s].
//
//   similarity_kernel   one thread per matrix element of the pool
//   HOTA   sums_kernel        row / column sums of every matrix (one thread per box, sequential in slot order)
//          pass1_kernel       one wave per ground-truth id walks the sequence's frames IN ORDER; the lanes take the frame's
//                             predictions and add sim_iou into the id's row of `potential`: frame order per pair, no atomics
//          score_kernel       -(gas * s) per element, gas formed on the fly from potential and the counts
//          assign_kernel      one wave per frame: lsap_problem
//          tally_kernel       one thread per (frame, alpha): the frame's matches in slot order -> count, sum, matches[pair][alpha] (integer atomics)
//          rows_kernel        one wave per ground-truth id: lane (kind, alpha) sums its row in ascending tracker id
//          hota_final_kernel  one wave per sequence: lane alpha adds the frames in order, the rows in ascending ground-truth id
//   CLEAR  clear_kernel       one wave per sequence walks its frames: score matrix in workspace, lsap_problem, the state update
//   Identity  pm_kernel (one thread per element, integer atomics), identity_kernel (one wave per sequence: the (G + T)^2 matrix, lsap_problem)
// Every status is a word per sequence: 0, or the solver's LSAP_* (3: too large — for Identity the caller's cue to solve that one on the
// host), or MOT_BAD_TABLE when the tables contradict each other (nothing is indexed with such a table).  Nothing here synchronises the device.
#include "cnl_common.h"

#pragma clang fp contract(off)   // one rounding per operation (the only fused multiply-adds left are inside the IEEE division sequence)

#include "lsap_device.h"

namespace cnl_mot {
using namespace cnl_track;

constexpr int NA = 19;                      // alpha = 0.05 .. 0.95
constexpr int NK = 3 * NA;                  // AssA | AssRe | AssPr per alpha
constexpr double EPS = 0x1p-52;             // np.finfo(float).eps
constexpr int ID_MAX = LSAP_MAX_SHORT;      // Identity: G + T of a sequence solved here
constexpr int MOT_BAD_TABLE = 5;
constexpr int NONE = -1;

typedef cnl_mot_tables Tab;

__device__ __forceinline__ double similarity(const double* __restrict__ g, const double* __restrict__ d) {
    const double x0g = g[0], y0g = g[1], x1g = g[0] + g[2], y1g = g[1] + g[3];
    const double x0d = d[0], y0d = d[1], x1d = d[0] + d[2], y1d = d[1] + d[3];
    const double iw = fmax(fmin(x1g, x1d) - fmax(x0g, x0d), 0.0), ih = fmax(fmin(y1g, y1d) - fmax(y0g, y0d), 0.0);
    const double I = iw * ih;
    const double ag = (x1g - x0g) * (y1g - y0g), ad = (x1d - x0d) * (y1d - y0d);
    const double U = (ag + ad) - I;
    return (ag <= EPS || ad <= EPS || U <= EPS) ? 0.0 : I / U;
}

// the last f in 0..F-1 with off[f] <= p (off ascending, off[0] <= p < off[F]): the frame that owns pooled element p
__device__ __forceinline__ int owner(const int64_t* __restrict__ off, int F, long long p) {
    int lo = 0, hi = F;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// One frame's place in the pools, checked against the pools' sizes.
struct Frame {
    long long go, po, so;
    int ng, np;
    bool ok;
};
__device__ __forceinline__ Frame frame_at(const Tab& t, int f) {
    Frame r;
    r.go = t.gt_off[f]; r.po = t.pr_off[f]; r.so = t.sim_off[f];
    const long long ng = t.gt_off[f + 1] - r.go, np = t.pr_off[f + 1] - r.po;
    r.ok = r.go >= 0 && r.po >= 0 && r.so >= 0 && ng >= 0 && np >= 0 && ng <= LSAP_MAX_LONG && np <= LSAP_MAX_LONG && r.go + ng <= t.n_gt &&
           r.po + np <= t.n_pr && t.sim_off[f + 1] - r.so == ng * np && r.so + ng * np <= t.sim_total;
    r.ng = r.ok ? (int)ng : 0;
    r.np = r.ok ? (int)np : 0;
    return r;
}
// One sequence's place.
struct Seq {
    long long f0, f1, g0, t0, pair0;
    int G, T;
    bool ok;
};
__device__ __forceinline__ Seq seq_at(const Tab& t, int s) {
    Seq r;
    r.f0 = t.seq_frm[s]; r.f1 = t.seq_frm[s + 1]; r.g0 = t.seq_gid[s]; r.t0 = t.seq_tid[s]; r.pair0 = t.seq_pair[s];
    const long long G = t.seq_gid[s + 1] - r.g0, T = t.seq_tid[s + 1] - r.t0;
    r.ok = r.f0 >= 0 && r.f1 >= r.f0 && r.f1 <= t.F && r.g0 >= 0 && r.t0 >= 0 && G >= 0 && T >= 0 && G < (1ll << 31) && T < (1ll << 31) &&
           r.g0 + G <= t.sum_g && r.t0 + T <= t.sum_t && r.pair0 >= 0 && t.seq_pair[s + 1] - r.pair0 == G * T && r.pair0 + G * T <= t.pair_total;
    r.G = r.ok ? (int)G : 0;
    r.T = r.ok ? (int)T : 0;
    return r;
}
// Element p of the similarity pool: its frame, slots, ids and pair.
struct Elem {
    Frame fr;
    Seq sq;
    int f, i, j, gid, tid;
    long long pair;
    bool ok;
};
__device__ __forceinline__ Elem elem_at(const Tab& t, long long p, bool with_ids) {
    Elem e;
    e.f = owner(t.sim_off, (int)t.F, p);
    e.fr = frame_at(t, e.f);
    const long long q = p - e.fr.so;
    e.ok = e.fr.ok && e.fr.np > 0 && q >= 0 && q < (long long)e.fr.ng * e.fr.np;
    e.i = e.ok ? (int)(q / e.fr.np) : 0;
    e.j = e.ok ? (int)(q - (long long)e.i * e.fr.np) : 0;
    e.gid = e.tid = 0;
    e.pair = 0;
    if (e.ok && with_ids) {
        const int s = t.frm_seq[e.f];
        e.ok = s >= 0 && s < t.S;
        if (e.ok) {
            e.sq = seq_at(t, s);
            e.gid = t.gt_ids[e.fr.go + e.i];
            e.tid = t.pr_ids[e.fr.po + e.j];
            e.ok = e.sq.ok && e.f >= e.sq.f0 && e.f < e.sq.f1 && e.gid >= 0 && e.gid < e.sq.G && e.tid >= 0 && e.tid < e.sq.T;
            e.pair = e.sq.pair0 + (long long)e.gid * e.sq.T + e.tid;
        }
    }
    return e;
}

__global__ __launch_bounds__(256) void similarity_kernel(const Tab t, double* __restrict__ sim) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= t.sim_total) return;
    const Elem e = elem_at(t, p, false);
    if (!e.ok) return;
    sim[p] = similarity(t.gt_boxes + (e.fr.go + e.i) * 4, t.pr_boxes + (e.fr.po + e.j) * 4);
}

// ---------------------------------------------------------------------------------------------------------------- HOTA
// Workspace: f64 rsum[n_gt] | csum[n_pr] | potential[pairs] | score[sim_total] | fsum[F][19] | rowsum[sum_g][57] |
//            i32 matches[pairs][19] | col[n_gt] | fcnt[F][19] | fstatus[F]
struct HotaWs {
    double *rsum, *csum, *potential, *score, *fsum, *rowsum;
    int *matches, *col, *fcnt, *fstatus;
};
__host__ __device__ inline HotaWs hota_ws(char* ws, const Tab& t) {
    HotaWs w;
    double* d = reinterpret_cast<double*>(ws);
    w.rsum = d; d += t.n_gt;
    w.csum = d; d += t.n_pr;
    w.potential = d; d += t.pair_total;
    w.score = d; d += t.sim_total;
    w.fsum = d; d += t.F * NA;
    w.rowsum = d; d += t.sum_g * NK;
    int* i = reinterpret_cast<int*>(d);
    w.matches = i; i += t.pair_total * NA;
    w.col = i; i += t.n_gt;
    w.fcnt = i; i += t.F * NA;
    w.fstatus = i; i += t.F;
    return w;
}
__host__ __device__ inline long long hota_ws_bytes(const Tab& t) {
    const long long f64 = t.n_gt + t.n_pr + t.pair_total + t.sim_total + t.F * NA + t.sum_g * NK;
    const long long i32 = t.pair_total * NA + t.n_gt + t.F * NA + t.F;
    return 8 * f64 + ((4 * i32 + 7) & ~7ll);
}

__global__ __launch_bounds__(256) void sums_kernel(const Tab t, const double* __restrict__ sim, double* __restrict__ rsum, double* __restrict__ csum) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x < t.n_gt) {
        const int f = owner(t.gt_off, (int)t.F, x);
        const Frame fr = frame_at(t, f);
        const long long i = x - fr.go;
        double r = 0.0;
        if (fr.ok && i >= 0 && i < fr.ng)
            for (int j = 0; j < fr.np; ++j) r = r + sim[fr.so + i * fr.np + j];
        rsum[x] = r;
    } else if (x < t.n_gt + t.n_pr) {
        const long long y = x - t.n_gt;
        const int f = owner(t.pr_off, (int)t.F, y);
        const Frame fr = frame_at(t, f);
        const long long j = y - fr.po;
        double c = 0.0;
        if (fr.ok && j >= 0 && j < fr.np)
            for (int i = 0; i < fr.ng; ++i) c = c + sim[fr.so + (long long)i * fr.np + j];
        csum[y] = c;
    }
}

// the slot of id `g` among the frame's ground truths, or -1 (uniform)
__device__ __forceinline__ int slot_of(const int32_t* __restrict__ ids, const Frame& fr, int g) {
    const int lane = threadIdx.x;
    for (int i0 = 0; i0 < fr.ng; i0 += 64) {
        const int i = i0 + lane;
        const unsigned long long m = __ballot(i < fr.ng && ids[fr.go + i] == g);
        if (m) return i0 + __ffsll((long long)m) - 1;
    }
    return -1;
}

// grid (max G, S), one wave: ground-truth id blockIdx.x of sequence blockIdx.y
__global__ __launch_bounds__(64) void pass1_kernel(const Tab t, const double* __restrict__ sim, const double* __restrict__ rsum,
                                                   const double* __restrict__ csum, double* potential) {
    const int lane = threadIdx.x, g = blockIdx.x;
    const Seq sq = seq_at(t, blockIdx.y);
    if (!sq.ok || g >= sq.G) return;
    double* const row = potential + sq.pair0 + (long long)g * sq.T;
    for (long long f = sq.f0; f < sq.f1; ++f) {
        const Frame fr = frame_at(t, (int)f);
        if (fr.ng == 0 || fr.np == 0) continue;
        const int slot = slot_of(t.gt_ids, fr, g);
        if (slot < 0) continue;
        const double r = rsum[fr.go + slot];
        for (int j = lane; j < fr.np; j += 64) {
            const double s = sim[fr.so + (long long)slot * fr.np + j];
            if (s > 0.0) {                                   // (a zero adds +0.0: no bit changes)
                const double den = (csum[fr.po + j] + r) - s;
                const double v = den > EPS ? s / den : 0.0;
                const int tid = t.pr_ids[fr.po + j];
                if (tid >= 0 && tid < sq.T) row[tid] = row[tid] + v;
            }
        }
        __syncthreads();      // a pair's next contribution may come from another lane: this frame's stores before the next frame's loads
    }
}

__global__ __launch_bounds__(256) void score_kernel(const Tab t, const double* __restrict__ sim, const double* __restrict__ potential,
                                                    double* __restrict__ score) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= t.sim_total) return;
    const Elem e = elem_at(t, p, true);
    if (!e.ok) { score[p] = __builtin_nan(""); return; }      // (the solver refuses the frame: LSAP_INVALID)
    const double pot = potential[e.pair];
    const double gas = pot / (((double)t.gt_count[e.sq.g0 + e.gid] + (double)t.pr_count[e.sq.t0 + e.tid]) - pot);
    score[p] = -(gas * sim[p]);
}

__global__ __launch_bounds__(64) void assign_kernel(const Tab t, const double* __restrict__ score, int* __restrict__ col, int* __restrict__ fstatus,
                                                    int nr_cap, int nc_cap) {
    extern __shared__ double lsap_lds[];
    const int f = blockIdx.x;
    const Frame fr = frame_at(t, f);
    int st = fr.ok ? LSAP_OK : MOT_BAD_TABLE;
    if (fr.ng > 0 && fr.np > 0) st = lsap_problem(score + fr.so, fr.np, fr.ng, fr.np, nr_cap, nc_cap, lsap_carve(lsap_lds, nr_cap, nc_cap), col + fr.go);
    if (threadIdx.x == 0) fstatus[f] = st;
}

// thread (frame, alpha): 32 threads per frame, 19 of them at work
__global__ __launch_bounds__(64) void tally_kernel(const Tab t, const double* __restrict__ sim, const double* __restrict__ alpha,
                                                   const int* __restrict__ col, const int* __restrict__ fstatus, int* matches,
                                                   double* __restrict__ fsum, int* __restrict__ fcnt) {
    const long long x = (long long)blockIdx.x * 64 + threadIdx.x;
    const int f = (int)(x >> 5), a = (int)(x & 31);
    if (f >= t.F || a >= NA) return;
    const Frame fr = frame_at(t, f);
    int cnt = 0;
    double sum = 0.0;
    const int s = t.frm_seq[f];
    if (fr.ng > 0 && fr.np > 0 && fstatus[f] == LSAP_OK && s >= 0 && s < t.S) {
        const Seq sq = seq_at(t, s);
        const double bar = alpha[a] - EPS;
        for (int i = 0; i < fr.ng; ++i) {
            const int c = col[fr.go + i];
            if (c < 0 || c >= fr.np) continue;
            const double v = sim[fr.so + (long long)i * fr.np + c];
            if (!(v >= bar)) continue;
            ++cnt;
            sum = sum + v;
            const int gid = t.gt_ids[fr.go + i], tid = t.pr_ids[fr.po + c];
            if (sq.ok && gid >= 0 && gid < sq.G && tid >= 0 && tid < sq.T) atomicAdd(&matches[(sq.pair0 + (long long)gid * sq.T + tid) * NA + a], 1);
        }
    }
    fcnt[(long long)f * NA + a] = cnt;
    fsum[(long long)f * NA + a] = sum;
}

// grid (max G, S), one wave: lane = kind * 19 + alpha sums row g of sequence blockIdx.y in ascending tracker id
__global__ __launch_bounds__(64) void rows_kernel(const Tab t, const int* __restrict__ matches, double* __restrict__ rowsum) {
    const int lane = threadIdx.x, g = blockIdx.x;
    const Seq sq = seq_at(t, blockIdx.y);
    if (!sq.ok || g >= sq.G || lane >= NK) return;
    const int kind = lane / NA, a = lane - kind * NA;
    const double gc = (double)t.gt_count[sq.g0 + g];
    const int* const m_row = matches + (sq.pair0 + (long long)g * sq.T) * NA + a;
    double row = 0.0;
    for (int tid = 0; tid < sq.T; ++tid) {
        const int m = m_row[(long long)tid * NA];
        if (m <= 0) continue;                                 // (a zero adds +0.0)
        const double x = (double)m, tc = (double)t.pr_count[sq.t0 + tid];
        const double d = kind == 0 ? fmax(1.0, (gc + tc) - x) : kind == 1 ? fmax(1.0, gc) : fmax(1.0, tc);
        row = row + x * (x / d);
    }
    rowsum[(sq.g0 + g) * NK + lane] = row;
}

// one wave per sequence.  out_f64 [S][4][19]: LocA_sum, AssA, AssRe, AssPr; out_i64 [S][3][19]: TP, FN, FP
__global__ __launch_bounds__(64) void hota_final_kernel(const Tab t, const double* __restrict__ fsum, const int* __restrict__ fcnt,
                                                        const int* __restrict__ fstatus, const double* __restrict__ rowsum,
                                                        double* __restrict__ out_f64, long long* __restrict__ out_i64, int* __restrict__ status) {
    const int lane = threadIdx.x, s = blockIdx.x;
    const Seq sq = seq_at(t, s);
    const int kind = lane / NA, a = lane - kind * NA;
    long long tp = 0, fn = 0, fp = 0;
    double loc = 0.0;
    int st = sq.ok ? LSAP_OK : MOT_BAD_TABLE;
    if (sq.ok && lane < NA)
        for (long long f = sq.f0; f < sq.f1; ++f) {
            const Frame fr = frame_at(t, (int)f);
            const int c = fcnt[f * NA + a], fs = fstatus[f];
            st = fs > st ? fs : st;
            tp += c; fn += fr.ng - c; fp += fr.np - c;
            loc = loc + fsum[f * NA + a];
        }
    const long long tp_a = __shfl(tp, a < NA ? a : 0);
    if (lane >= NK) return;
    double acc = 0.0;
    for (int g = 0; g < sq.G; ++g) acc = acc + rowsum[(sq.g0 + g) * NK + lane];
    out_f64[((long long)s * 4 + 1 + kind) * NA + a] = acc / fmax(1.0, (double)tp_a);
    if (lane < NA) {
        out_f64[(long long)s * 4 * NA + a] = loc;
        out_i64[((long long)s * 3 + 0) * NA + a] = tp;
        out_i64[((long long)s * 3 + 1) * NA + a] = fn;
        out_i64[((long long)s * 3 + 2) * NA + a] = fp;
        if (lane == 0) status[s] = st;
    }
}

// ---------------------------------------------------------------------------------------------------------------- CLEAR
// Workspace: f64 mat[S][max_frame_pairs] | i32 prev[sum_g] | step_tid[sum_g] | step_at[sum_g] | matched[sum_g] | frag[sum_g]
// prev_step[gid] is "set" when step_at[gid] holds the number of the last frame that went through the assignment.
__host__ __device__ inline long long clear_ws_bytes(const Tab& t) { return 8 * t.S * t.max_frame_pairs + ((20 * t.sum_g + 7) & ~7ll); }

// out_i64 [S][8]: TP FN FP IDSW MT PT ML Frag; out_f64 [S]: MOTP_sum.  LDS: the solver's, then col[row_cap]
__global__ __launch_bounds__(64) void clear_kernel(const Tab t, const double* __restrict__ sim, char* ws, double* __restrict__ out_f64,
                                                   long long* __restrict__ out_i64, int* __restrict__ status, int nr_cap, int nc_cap) {
    extern __shared__ double lsap_lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    const Seq sq = seq_at(t, s);
    const LsapLds L = lsap_carve(lsap_lds, nr_cap, nc_cap);
    int* const col = reinterpret_cast<int*>(reinterpret_cast<char*>(lsap_lds) + lsap_lds_bytes(nr_cap, nc_cap));
    double* const mat = reinterpret_cast<double*>(ws) + (long long)s * t.max_frame_pairs;
    int* const ints = reinterpret_cast<int*>(ws + 8 * t.S * t.max_frame_pairs);
    int* const prev = ints + sq.g0;
    int* const step_tid = ints + t.sum_g + sq.g0;
    int* const step_at = ints + 2 * t.sum_g + sq.g0;
    int* const matched = ints + 3 * t.sum_g + sq.g0;
    int* const frag = ints + 4 * t.sum_g + sq.g0;
    long long tp = 0, fn = 0, fp = 0, idsw = 0;
    double motp = 0.0;
    int st = sq.ok ? LSAP_OK : MOT_BAD_TABLE;
    for (int g = lane; g < sq.G; g += 64) { prev[g] = NONE; step_tid[g] = NONE; step_at[g] = NONE; matched[g] = 0; frag[g] = 0; }
    __syncthreads();
    int last = 0;                                             // frames that went through the assignment so far
    for (long long f = sq.f0; f < sq.f1 && st == LSAP_OK; ++f) {
        const Frame fr = frame_at(t, (int)f);
        if (!fr.ok || (long long)fr.ng * fr.np > t.max_frame_pairs) { st = MOT_BAD_TABLE; break; }
        if (fr.ng == 0) { fp += fr.np; continue; }            // the state is not touched
        if (fr.np == 0) { fn += fr.ng; continue; }
        const int total = fr.ng * fr.np;
        for (int p = lane; p < total; p += 64) {
            const int i = p / fr.np, j = p - i * fr.np;
            const int gid = t.gt_ids[fr.go + i], tid = t.pr_ids[fr.po + j];
            const double v = sim[fr.so + p];
            const bool in = gid >= 0 && gid < sq.G;
            const bool same = in && last > 0 && step_at[gid] == last - 1 && step_tid[gid] == tid;
            const double score = v < 0.5 - EPS ? 0.0 : (same ? 1000.0 + v : v);
            mat[p] = in ? -score : __builtin_nan("");
        }
        __syncthreads();
        st = lsap_problem(mat, fr.np, fr.ng, fr.np, nr_cap, nc_cap, L, col);
        __syncthreads();
        if (st != LSAP_OK) break;
        double frame_sum = 0.0;
        for (int i0 = 0; i0 < fr.ng; i0 += 64) {
            const int i = i0 + lane;
            bool kept = false, sw = false;
            double v = 0.0;
            if (i < fr.ng) {
                const int c = col[i];
                if (c >= 0 && c < fr.np && -mat[(long long)i * fr.np + c] > EPS) {
                    kept = true;
                    const int gid = t.gt_ids[fr.go + i], tid = t.pr_ids[fr.po + c];      // (gid is in range: the matrix's row would be NaN)
                    v = sim[fr.so + (long long)i * fr.np + c];
                    const int before = prev[gid];
                    sw = before != NONE && before != tid;
                    matched[gid] += 1;
                    if (!(last > 0 && step_at[gid] == last - 1)) frag[gid] += 1;
                    prev[gid] = tid; step_tid[gid] = tid; step_at[gid] = last;
                }
            }
            idsw += __popcll(__ballot(sw));
            unsigned long long m = __ballot(kept);
            const int n = __popcll(m);
            tp += n;
            while (m) {                                       // the frame's sum in ascending ground-truth slot (uniform)
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                frame_sum = frame_sum + __shfl(v, src);
            }
        }
        motp = motp + frame_sum;
        ++last;
        __syncthreads();      // the state's stores before the next frame's loads, which other lanes issue
    }
    // every frame's matches are counted in tp; FN and FP follow from the totals of the frames that held both sides
    long long n_gt_both = 0, n_pr_both = 0;
    if (st == LSAP_OK)
        for (long long f = sq.f0 + lane; f < sq.f1; f += 64) {
            const Frame fr = frame_at(t, (int)f);
            if (fr.ng > 0 && fr.np > 0) { n_gt_both += fr.ng; n_pr_both += fr.np; }
        }
    int mt = 0, pt = 0, fragments = 0;
    for (int g = lane; g < sq.G; g += 64) {
        const int gc = t.gt_count[sq.g0 + g], fc = frag[g];
        if (gc > 0) {
            const double ratio = (double)matched[g] / (double)gc;
            mt += ratio > 0.8;
            pt += ratio >= 0.2;
        }
        if (fc > 0) fragments += fc - 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_gt_both += __shfl_xor(n_gt_both, o); n_pr_both += __shfl_xor(n_pr_both, o);
        mt += __shfl_xor(mt, o); pt += __shfl_xor(pt, o); fragments += __shfl_xor(fragments, o);
    }
    if (lane == 0) {
        const bool ok = st == LSAP_OK;
        long long* o = out_i64 + (long long)s * 8;
        o[0] = ok ? tp : 0; o[1] = ok ? fn + (n_gt_both - tp) : 0; o[2] = ok ? fp + (n_pr_both - tp) : 0; o[3] = ok ? idsw : 0;
        o[4] = ok ? mt : 0; o[5] = ok ? pt - mt : 0; o[6] = ok ? sq.G - pt : 0; o[7] = ok ? fragments : 0;
        out_f64[s] = ok ? motp : 0.0;
        status[s] = st;
    }
}

// ---------------------------------------------------------------------------------------------------------------- Identity
__global__ __launch_bounds__(256) void pm_kernel(const Tab t, const double* __restrict__ sim, int* pm) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= t.sim_total) return;
    if (!(sim[p] >= 0.5)) return;
    const Elem e = elem_at(t, p, true);
    if (e.ok) atomicAdd(&pm[e.pair], 1);
}

// entry (i, c) of fn and fp (G + T square)
__device__ __forceinline__ void id_entry(const Tab& t, const Seq& sq, const int* pm, int i, int c, double& fn, double& fp) {
    fn = 0.0; fp = 0.0;
    if (i < sq.G) {
        const double gc = (double)t.gt_count[sq.g0 + i];
        if (c < sq.T) {
            const double m = (double)pm[sq.pair0 + (long long)i * sq.T + c];
            fn = gc - m;
            fp = (double)t.pr_count[sq.t0 + c] - m;
        } else {
            fn = c - sq.T == i ? gc : 1e10;
        }
    } else if (c < sq.T) {
        fp = i - sq.G == c ? (double)t.pr_count[sq.t0 + c] : 1e10;
    }
}

// Workspace: f64 mat[id_total], sequence s at seq_idm[s] (its (G + T)^2 entries; none when G + T > 1024).  out_i64 [S][2]: IDFN, IDFP
__global__ __launch_bounds__(64) void identity_kernel(const Tab t, const int* pm, double* mat_pool, long long* __restrict__ out_i64,
                                                      int* __restrict__ status, int cap) {
    extern __shared__ double lsap_lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    const Seq sq = seq_at(t, s);
    const long long N = (long long)sq.G + sq.T, m0 = t.seq_idm[s];
    int st = !sq.ok ? MOT_BAD_TABLE : N > cap ? LSAP_TOO_LARGE : (m0 < 0 || t.seq_idm[s + 1] - m0 != N * N || m0 + N * N > t.id_total) ? MOT_BAD_TABLE : LSAP_OK;
    double fn_sum = 0.0, fp_sum = 0.0;
    if (st == LSAP_OK && N > 0) {
        const int n = (int)N;
        double* const mat = mat_pool + m0;
        int* const col = reinterpret_cast<int*>(reinterpret_cast<char*>(lsap_lds) + lsap_lds_bytes(cap, cap));
        for (int p = lane; p < n * n; p += 64) {
            const int i = p / n, c = p - i * n;
            double fn, fp;
            id_entry(t, sq, pm, i, c, fn, fp);
            mat[p] = fn + fp;
        }
        __syncthreads();
        st = lsap_problem(mat, n, n, n, cap, cap, lsap_carve(lsap_lds, cap, cap), col);
        __syncthreads();
        if (st == LSAP_OK)
            for (int i = lane; i < n; i += 64) {
                const int c = col[i];
                if (c < 0 || c >= n) continue;
                double fn, fp;
                id_entry(t, sq, pm, i, c, fn, fp);
                fn_sum += fn; fp_sum += fp;                  // integers below 2^53: exact in any order
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { fn_sum += __shfl_xor(fn_sum, o); fp_sum += __shfl_xor(fp_sum, o); }
    if (lane == 0) {
        out_i64[2 * (long long)s] = st == LSAP_OK ? (long long)fn_sum : 0;
        out_i64[2 * (long long)s + 1] = st == LSAP_OK ? (long long)fp_sum : 0;
        status[s] = st;
    }
}

static cnl::DeviceOnce assign_once, clear_once, identity_once;
constexpr int LSAP_LDS_MAX = 12 * LSAP_MAX_SHORT + 28 * LSAP_MAX_LONG;
constexpr int CLEAR_LDS_MAX = LSAP_LDS_MAX + 4 * LSAP_MAX_LONG;
constexpr int IDENTITY_LDS_MAX = 44 * ID_MAX;

static inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The tables as far as the host can judge them (the device checks every offset it reads against the pools' sizes).
static int check_tables(const Tab* t, const char* who, bool need_ids) {
    CNL_REQUIRE(t, CNL_E_BAD_ARG, "%s: null tables", who);
    CNL_REQUIRE(t->F >= 0 && t->F < (1ll << 26) && t->S >= 1 && t->S <= 65535, CNL_E_BAD_ARG, "%s: F = %lld outside 0..2^26-1 or S = %lld outside 1..65535",
                who, (long long)t->F, (long long)t->S);
    CNL_REQUIRE(t->n_gt >= 0 && t->n_pr >= 0 && t->sim_total >= 0 && t->pair_total >= 0 && t->sum_g >= 0 && t->sum_t >= 0 && t->max_gids >= 0 &&
                    t->max_gt_frame >= 0 && t->max_pr_frame >= 0 && t->max_frame_pairs >= 0 && t->id_total >= 0, CNL_E_BAD_ARG, "%s: a negative size", who);
    CNL_REQUIRE(t->n_gt < (1ll << 31) && t->n_pr < (1ll << 31) && t->sim_total < (1ll << 40) && t->pair_total < (1ll << 40) && t->sum_g < (1ll << 31) &&
                    t->sum_t < (1ll << 31) && t->max_gids <= t->sum_g && t->id_total < (1ll << 40), CNL_E_BAD_ARG, "%s: a size out of range", who);
    CNL_REQUIRE(t->max_gt_frame <= t->n_gt && t->max_pr_frame <= t->n_pr && t->max_frame_pairs <= t->sim_total &&
                    t->max_frame_pairs <= t->max_gt_frame * t->max_pr_frame, CNL_E_BAD_ARG, "%s: the per-frame maxima contradict the totals", who);
    CNL_REQUIRE(t->gt_off && t->pr_off && t->sim_off && t->seq_frm && t->seq_gid && t->seq_tid && t->seq_pair && t->seq_idm, CNL_E_BAD_ARG,
                "%s: null offset table", who);
    CNL_REQUIRE((t->F == 0 || t->frm_seq) && (t->n_gt == 0 || (t->gt_boxes && (!need_ids || t->gt_ids))) && (t->n_pr == 0 || (t->pr_boxes && (!need_ids || t->pr_ids))) &&
                    (!need_ids || ((t->sum_g == 0 || t->gt_count) && (t->sum_t == 0 || t->pr_count))), CNL_E_BAD_ARG, "%s: null pointer", who);
    CNL_REQUIRE(aligned(t->gt_boxes, 8) && aligned(t->pr_boxes, 8) && aligned(t->gt_off, 8) && aligned(t->pr_off, 8) && aligned(t->sim_off, 8) &&
                    aligned(t->seq_frm, 8) && aligned(t->seq_gid, 8) && aligned(t->seq_tid, 8) && aligned(t->seq_pair, 8) && aligned(t->seq_idm, 8) &&
                    aligned(t->gt_ids, 4) && aligned(t->pr_ids, 4) && aligned(t->frm_seq, 4) && aligned(t->gt_count, 4) && aligned(t->pr_count, 4),
                CNL_E_BAD_ARG, "%s: the 64-bit arrays must be 8-byte aligned, the 32-bit ones 4-byte aligned", who);
    const long long lo = t->max_gt_frame < t->max_pr_frame ? t->max_gt_frame : t->max_pr_frame;
    const long long hi = t->max_gt_frame < t->max_pr_frame ? t->max_pr_frame : t->max_gt_frame;
    CNL_REQUIRE(lo <= LSAP_MAX_SHORT && hi <= LSAP_MAX_LONG, CNL_E_UNSUPPORTED,
                "%s: a frame of %lld ground truths x %lld predictions: at most %d on the smaller side and %d on the larger are supported", who,
                (long long)t->max_gt_frame, (long long)t->max_pr_frame, LSAP_MAX_SHORT, LSAP_MAX_LONG);
    return CNL_OK;
}
static inline void caps(const Tab* t, int& nr_cap, int& nc_cap) {
    const int lo = (int)(t->max_gt_frame < t->max_pr_frame ? t->max_gt_frame : t->max_pr_frame);
    const int hi = (int)(t->max_gt_frame < t->max_pr_frame ? t->max_pr_frame : t->max_gt_frame);
    nr_cap = lo > 0 ? lo : 1;
    nc_cap = hi > 0 ? hi : 1;
}
static inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace cnl_mot
using namespace cnl_mot;

extern "C" int cnl_mot_similarity_f64(const cnl_mot_tables* tables, double* sim, void* stream) {
    if (int rc = check_tables(tables, "cnl_mot_similarity_f64", false)) return rc;
    if (tables->sim_total == 0) return CNL_OK;
    CNL_REQUIRE(sim && aligned(sim, 8), CNL_E_BAD_ARG, "cnl_mot_similarity_f64: sim must be an 8-byte aligned pointer");
    hipLaunchKernelGGL(similarity_kernel, dim3(blocks(tables->sim_total, 256)), dim3(256), 0, (hipStream_t)stream, *tables, sim);
    return cnl::check_launch("mot_eval similarity_kernel");
}

extern "C" int64_t cnl_mot_hota_workspace_bytes(const cnl_mot_tables* tables) {
    if (!tables || check_tables(tables, "cnl_mot_hota_workspace_bytes", false)) return 0;
    return hota_ws_bytes(*tables);
}

extern "C" int cnl_mot_hota_f64(const cnl_mot_tables* tables, const double* sim, const double* alpha, double* out_f64, int64_t* out_i64,
                                int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_tables(tables, "cnl_mot_hota_f64", true)) return rc;
    const Tab& t = *tables;
    CNL_REQUIRE(alpha && out_f64 && out_i64 && status && workspace && (t.sim_total == 0 || sim), CNL_E_BAD_ARG, "cnl_mot_hota_f64: null pointer");
    CNL_REQUIRE(aligned(sim, 8) && aligned(alpha, 8) && aligned(out_f64, 8) && aligned(out_i64, 8) && aligned(status, 4) && aligned(workspace, 8),
                CNL_E_BAD_ARG, "cnl_mot_hota_f64: sim, alpha, out_f64, out_i64 and workspace must be 8-byte aligned, status 4-byte aligned");
    const HotaWs w = hota_ws((char*)workspace, t);
    const long long need = hota_ws_bytes(t);
    CNL_REQUIRE(workspace_bytes >= need, CNL_E_BAD_ARG, "cnl_mot_hota_f64: workspace holds %lld bytes, these tables need %lld (cnl_mot_hota_workspace_bytes)",
                (long long)workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    int nr_cap, nc_cap;
    caps(tables, nr_cap, nc_cap);
    if (int rc = cnl::kernel_setup(assign_once, (const void*)assign_kernel, LSAP_LDS_MAX)) return rc;
    if (t.pair_total > 0) {
        CNL_HIP(hipMemsetAsync(w.potential, 0, 8 * t.pair_total, st));
        CNL_HIP(hipMemsetAsync(w.matches, 0, 4 * NA * t.pair_total, st));
    }
    if (t.n_gt + t.n_pr > 0) {
        hipLaunchKernelGGL(sums_kernel, dim3(blocks(t.n_gt + t.n_pr, 256)), dim3(256), 0, st, t, sim, w.rsum, w.csum);
        if (int rc = cnl::check_launch("mot_eval sums_kernel")) return rc;
    }
    if (t.sim_total > 0 && t.max_gids > 0) {
        hipLaunchKernelGGL(pass1_kernel, dim3((unsigned)t.max_gids, (unsigned)t.S), dim3(64), 0, st, t, sim, w.rsum, w.csum, w.potential);
        if (int rc = cnl::check_launch("mot_eval pass1_kernel")) return rc;
        hipLaunchKernelGGL(score_kernel, dim3(blocks(t.sim_total, 256)), dim3(256), 0, st, t, sim, w.potential, w.score);
        if (int rc = cnl::check_launch("mot_eval score_kernel")) return rc;
    }
    if (t.F > 0) {
        hipLaunchKernelGGL(assign_kernel, dim3((unsigned)t.F), dim3(64), lsap_lds_bytes(nr_cap, nc_cap), st, t, w.score, w.col, w.fstatus, nr_cap, nc_cap);
        if (int rc = cnl::check_launch("mot_eval assign_kernel")) return rc;
        hipLaunchKernelGGL(tally_kernel, dim3(blocks(t.F * 32, 64)), dim3(64), 0, st, t, sim, alpha, w.col, w.fstatus, w.matches, w.fsum, w.fcnt);
        if (int rc = cnl::check_launch("mot_eval tally_kernel")) return rc;
    }
    if (t.max_gids > 0) {
        hipLaunchKernelGGL(rows_kernel, dim3((unsigned)t.max_gids, (unsigned)t.S), dim3(64), 0, st, t, w.matches, w.rowsum);
        if (int rc = cnl::check_launch("mot_eval rows_kernel")) return rc;
    }
    hipLaunchKernelGGL(hota_final_kernel, dim3((unsigned)t.S), dim3(64), 0, st, t, w.fsum, w.fcnt, w.fstatus, w.rowsum, out_f64,
                       reinterpret_cast<long long*>(out_i64), status);
    return cnl::check_launch("mot_eval hota_final_kernel");
}

extern "C" int64_t cnl_mot_clear_workspace_bytes(const cnl_mot_tables* tables) {
    if (!tables || check_tables(tables, "cnl_mot_clear_workspace_bytes", false)) return 0;
    return clear_ws_bytes(*tables);
}

extern "C" int cnl_mot_clear_f64(const cnl_mot_tables* tables, const double* sim, double* out_f64, int64_t* out_i64, int32_t* status,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_tables(tables, "cnl_mot_clear_f64", true)) return rc;
    const Tab& t = *tables;
    const int64_t need = clear_ws_bytes(t);
    CNL_REQUIRE(out_f64 && out_i64 && status && (need == 0 || workspace) && (t.sim_total == 0 || sim), CNL_E_BAD_ARG, "cnl_mot_clear_f64: null pointer");
    CNL_REQUIRE(aligned(sim, 8) && aligned(out_f64, 8) && aligned(out_i64, 8) && aligned(status, 4) && aligned(workspace, 8), CNL_E_BAD_ARG,
                "cnl_mot_clear_f64: sim, out_f64, out_i64 and workspace must be 8-byte aligned, status 4-byte aligned");
    CNL_REQUIRE(workspace_bytes >= need, CNL_E_BAD_ARG, "cnl_mot_clear_f64: workspace holds %lld bytes, these tables need %lld (cnl_mot_clear_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
    int nr_cap, nc_cap;
    caps(tables, nr_cap, nc_cap);
    const int row_cap = t.max_gt_frame > 0 ? (int)t.max_gt_frame : 1;
    if (int rc = cnl::kernel_setup(clear_once, (const void*)clear_kernel, CLEAR_LDS_MAX)) return rc;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)t.S), dim3(64), lsap_lds_bytes(nr_cap, nc_cap) + 4ul * row_cap, (hipStream_t)stream, t, sim,
                       (char*)workspace, out_f64, reinterpret_cast<long long*>(out_i64), status, nr_cap, nc_cap);
    return cnl::check_launch("mot_eval clear_kernel");
}

extern "C" int64_t cnl_mot_identity_workspace_bytes(const cnl_mot_tables* tables) {
    if (!tables || check_tables(tables, "cnl_mot_identity_workspace_bytes", false)) return 0;
    return 8 * tables->id_total;
}

extern "C" int cnl_mot_identity_f64(const cnl_mot_tables* tables, const double* sim, int32_t* pm, int64_t* out_i64, int32_t* status,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_tables(tables, "cnl_mot_identity_f64", true)) return rc;
    const Tab& t = *tables;
    CNL_REQUIRE(out_i64 && status && (t.pair_total == 0 || pm) && (t.id_total == 0 || workspace) && (t.sim_total == 0 || sim), CNL_E_BAD_ARG,
                "cnl_mot_identity_f64: null pointer");
    CNL_REQUIRE(aligned(sim, 8) && aligned(out_i64, 8) && aligned(status, 4) && aligned(pm, 4) && aligned(workspace, 8), CNL_E_BAD_ARG,
                "cnl_mot_identity_f64: sim, out_i64 and workspace must be 8-byte aligned, pm and status 4-byte aligned");
    CNL_REQUIRE(workspace_bytes >= 8 * t.id_total, CNL_E_BAD_ARG,
                "cnl_mot_identity_f64: workspace holds %lld bytes, these tables need %lld (cnl_mot_identity_workspace_bytes)", (long long)workspace_bytes,
                (long long)(8 * t.id_total));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = cnl::kernel_setup(identity_once, (const void*)identity_kernel, IDENTITY_LDS_MAX)) return rc;
    if (t.pair_total > 0) CNL_HIP(hipMemsetAsync(pm, 0, 4 * t.pair_total, st));
    if (t.sim_total > 0) {
        hipLaunchKernelGGL(pm_kernel, dim3(blocks(t.sim_total, 256)), dim3(256), 0, st, t, sim, pm);
        if (int rc = cnl::check_launch("mot_eval pm_kernel")) return rc;
    }
    // the solver's LDS is sized for the largest sequence that is solved here
    hipLaunchKernelGGL(identity_kernel, dim3((unsigned)t.S), dim3(64), 44ul * ID_MAX, st, t, pm, (double*)workspace, reinterpret_cast<long long*>(out_i64),
                       status, ID_MAX);
    return cnl::check_launch("mot_eval identity_kernel");
}
