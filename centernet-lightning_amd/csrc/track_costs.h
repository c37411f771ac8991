// track_costs.h — the device code that turns one frame's detections into association costs: the detection-threshold compaction and the
// per-pair re-ID (float64) / box (float32) costs.  Shared by track.hip (one stream per launch) and track_streams.hip (S streams per
// launch) so that both write bit-identical matrices: the integer decisions taken from them (thresholds, assignment) must not depend on
// which entry point computed them.
// GATED instantiations of the per-pair functions (cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32) apply the class and motion gates of
// the header's cnl_track_gate before the one store of each cost; the ungated instantiations carry none of that code.
#pragma once
#include "cnl_common.h"
#include <initializer_list>
#include "kalman_ldl.h"     // ldl4: the motion gate factors the filter's S as the filter does

#pragma clang fp contract(off)   // one rounding per operation, like numpy / scipy: the costs feed thresholds and the Hungarian step

namespace cnl_track {

constexpr int MAXK = 1024;     // detections per frame (decode's k limit)

// What pair_costs reads 16 bytes at a time: a box of either side (box_cost != 0) and, when E % 4 == 0, four embedding elements (seq_dots).  The
// launchers refuse anything less aligned — but only what a launch reads: without tracks (T == 0) there are no pairs and nothing is required.
constexpr const char* INPUTS_ALIGNED = "with tracks, det_box / trk_box (box_cost != 0) and, when E % 4 == 0, det_emb / trk_emb must be 16-byte aligned";
inline bool inputs_aligned(const float* det_emb, const float* det_box, const float* trk_emb, const float* trk_box, int E, int T, int box_cost) {
    if (T == 0) return true;
    const uintptr_t boxes = box_cost ? (uintptr_t)det_box | (uintptr_t)trk_box : 0, embs = (E & 3) == 0 ? (uintptr_t)det_emb | (uintptr_t)trk_emb : 0;
    return ((boxes | embs) & 15) == 0;
}

// The checks of a cnl_track_gate that both gated entries share (a null gate: every gate off); `thresholds`: the entry's own.
inline int check_gate(const char* name, const cnl_track_gate* gate, const float* det_box, std::initializer_list<double> thresholds) {
    if (gate == nullptr || (gate->trk_label == nullptr && gate->kx == nullptr && gate->kP == nullptr)) return CNL_OK;
    CNL_REQUIRE((gate->kx == nullptr) == (gate->kP == nullptr), CNL_E_BAD_ARG, "%s: gate kx and kP come together (both null: no motion gate)", name);
    CNL_REQUIRE((((uintptr_t)gate->kx | (uintptr_t)gate->kP) & 7) == 0 && ((uintptr_t)gate->trk_label & 3) == 0, CNL_E_BAD_ARG,
                "%s: gate kx / kP must be 8-byte aligned, trk_label 4-byte aligned", name);
    if (gate->kx != nullptr) {
        CNL_REQUIRE(((uintptr_t)det_box & 15) == 0, CNL_E_BAD_ARG, "%s: with the motion gate det_box must be 16-byte aligned", name);
        CNL_REQUIRE(gate->motion_gate >= 0.0 && gate->motion_gate < CNL_TRACK_GATE_COST, CNL_E_BAD_ARG,
                    "%s: motion_gate %g must lie in [0, %g)", name, gate->motion_gate, CNL_TRACK_GATE_COST);
        CNL_REQUIRE(gate->motion_weight >= 0.0 && gate->motion_weight <= 1.0, CNL_E_BAD_ARG, "%s: motion_weight %g must lie in [0, 1]", name,
                    gate->motion_weight);
    }
    for (const double t : thresholds)
        CNL_REQUIRE(!(t >= CNL_TRACK_GATE_COST), CNL_E_BAD_ARG, "%s: a threshold of %g would accept gated pairs (their cost is %g)", name, t,
                    CNL_TRACK_GATE_COST);
    return CNL_OK;
}

// numpy maximum/minimum propagate NaN (fmaxf/fminf do not)
__device__ __forceinline__ float np_max(float a, float b) { return (a != a) ? a : (b != b) ? b : (a > b ? a : b); }
__device__ __forceinline__ float np_min(float a, float b) { return (a != a) ? a : (b != b) ? b : (a < b ? a : b); }

// u.u, v.v and u.v in float64, each accumulated sequentially over e = 0..E-1 (scipy's dot order); the three chains are
// independent, so interleaving them hides the fp64 add latency without changing any result.
__device__ __forceinline__ void seq_dots(const float* __restrict__ u, const float* __restrict__ v, int E, double& uu, double& vv,
                                         double& uv) {
    uu = vv = uv = 0.0;
    int e = 0;
    if ((E & 3) == 0) {      // rows are 16-byte aligned when E % 4 == 0
        for (; e < E; e += 4) {
            const float4 a = *reinterpret_cast<const float4*>(u + e), b = *reinterpret_cast<const float4*>(v + e);
            const double a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w, b0 = b.x, b1 = b.y, b2 = b.z, b3 = b.w;
            uu = uu + a0 * a0; vv = vv + b0 * b0; uv = uv + a0 * b0;
            uu = uu + a1 * a1; vv = vv + b1 * b1; uv = uv + a1 * b1;
            uu = uu + a2 * a2; vv = vv + b2 * b2; uv = uv + a2 * b2;
            uu = uu + a3 * a3; vv = vv + b3 * b3; uv = uv + a3 * b3;
        }
    }
    for (; e < E; ++e) {
        const double a = u[e], b = v[e];
        uu = uu + a * a; vv = vv + b * b; uv = uv + a * b;
    }
}

// The (tiny) stable compaction {i : score[i] >= thr} — WINDOW: {i : thr <= score[i] < below} — into LDS, rebuilt by every workgroup: cheaper
// than a second launch.  Returns n.  (May be called again with the same wave_sum: every read of it lies before the closing barrier.)
template <bool WINDOW>
__device__ __forceinline__ int compact_scores_in(const float* __restrict__ det_score, const int k, const float thr, const float below, int* sel,
                                                 int* wave_sum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // thread t owns scores 4t..4t+3 (k <= 1024)
    int flag[4], cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid * 4 + i;
        flag[i] = idx < k && det_score[idx] >= thr && (!WINDOW || det_score[idx] < below);         // NaN compares false, as in numpy
        cnt += flag[i];
    }
    int incl = cnt;                                          // inclusive scan of cnt over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int base = 0, n = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += wave_sum[w];
        n += wave_sum[w];
    }
    int pos = base + incl - cnt;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (flag[i]) sel[pos++] = tid * 4 + i;
    __syncthreads();
    return n;
}
__device__ __forceinline__ int compact_scores(const float* __restrict__ det_score, const int k, const float thr, int* sel, int* wave_sum) {
    return compact_scores_in<false>(det_score, k, thr, 0.f, sel, wave_sum);
}

// Row mean in float64 in numpy's order (np.add.reduce over a contiguous last axis = pairwise summation: eight strided partial sums per block of <= 128 elements,
// combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the tail added sequentially; longer rows split in halves rounded down to a multiple of 8) — scipy's cdist
// "correlation" centres both operands with XA.mean(axis=1) before its cosine kernel.
__device__ double np_pairwise_sum(const float* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res = res + (double)a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (double)a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + (double)a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + (double)a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// Box distance of one (detection box, track box) pair: utils/box.py:49-92 in float32, numpy's operation order; box_mode 1 "iou", 2 "giou".
__device__ __forceinline__ float box_pair_cost(const float4 a, const float4 b, const int box_mode) {
    const float area1 = ((a.z - a.x) * (a.w - a.y));
    const float area2 = ((b.z - b.x) * (b.w - b.y));
    const float w = np_max((np_min(a.z, b.z) - np_max(a.x, b.x)), 0.f);
    const float h = np_max((np_min(a.w, b.w) - np_max(a.y, b.y)), 0.f);
    const float inter = (w * h);
    const float uni = ((area1 + area2) - inter);
    const float iou = (inter / uni);
    float score = iou;
    if (box_mode == 2) {
        const float wi = np_max((np_max(a.z, b.z) - np_min(a.x, b.x)), 0.f);
        const float hi = np_max((np_max(a.w, b.w) - np_min(a.y, b.y)), 0.f);
        const float hull = (wi * hi);
        score = (iou - ((hull - uni) / hull));
    }
    return (1.f - score);
}

// The gates of cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32 (include/centernet_gfx950.h: cnl_track_gate) as the cost functions read them:
// the table pointers start at the stream's first row, det_label at the launch's first detection and det0 is the first detection of the stream's slot.
constexpr double GATE_COST = CNL_TRACK_GATE_COST;
struct GateOps {
    const int* trk_label;      // null: no class gate
    const double *kx, *kP;     // null (together): no motion gate
    double motion_gate, motion_weight;
    const void* det_label;
    int label_kind;
    long det0;
};

// A detection's label as the records carry it (label_kind 1 int64, 2 int32, 3 float32 cast to int, 0: none = 0).
__device__ __forceinline__ int det_label_at(const void* __restrict__ det_label, const int label_kind, const long i) {
    return label_kind == 1 ? (int)reinterpret_cast<const long long*>(det_label)[i]
         : label_kind == 2 ? reinterpret_cast<const int*>(det_label)[i]
         : label_kind == 3 ? (int)reinterpret_cast<const float*>(det_label)[i] : 0;
}
__device__ __forceinline__ bool cross_class(const GateOps& g, const int d, const int t) {
    return g.trk_label != nullptr && det_label_at(g.det_label, g.label_kind, g.det0 + d) != g.trk_label[t];
}

// The motion gate of one pair (the header's rule): the squared Mahalanobis distance m of the detection's box z from track t's predicted state in
// the filter's own innovation metric S = P[:4, :4] + diag(r) = L D L' (kalman_ldl.h).  -> the stage-1 cost: GATE_COST outside the gate (a bad
// pivot and a NaN included), inside it reid (untouched bits) when motion_weight == 1, else motion_weight * reid + (1 - motion_weight) * m.
__device__ inline double motion_gated_cost(const double reid, const float4 zf, const double* __restrict__ x, const double* __restrict__ P,
                                                    const double motion_gate, const double motion_weight) {
    const double z[4] = {(double)zf.x, (double)zf.y, (double)zf.z, (double)zf.w};
    const double xs[4] = {x[0], x[1], x[2], x[3]};
    const double w = xs[2] - xs[0], h = xs[3] - xs[1];
    double r[4], y[4], L[4][4], dd[4], u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double q = ((i & 1) ? h : w) / 20.0;
        r[i] = q * q;
        y[i] = z[i] - xs[i];
    }
    const bool ok = cnl_kalman::ldl4([P](int i, int j) { return P[j * 8 + i]; }, r, L, dd);      // i >= j: the upper triangle, as the filter reads P
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double v = y[i];
        if (i > 0) {
            double acc = L[i][0] * u[0];
#pragma unroll
            for (int k = 1; k < i; ++k) acc = acc + L[i][k] * u[k];
            v = v - acc;
        }
        u[i] = v;
    }
    const double m = (((u[0] / dd[0]) * u[0] + (u[1] / dd[1]) * u[1]) + (u[2] / dd[2]) * u[2]) + (u[3] / dd[3]) * u[3];
    if (!ok || !(m <= motion_gate)) return GATE_COST;
    return motion_weight == 1.0 ? reid : motion_weight * reid + (1.0 - motion_weight) * m;
}

// Box costs alone of pair p = r * T + t of an n x T problem (the low-score stage: no re-ID matrix), written at box_cost[p].  GATED: a cross-class
// pair costs GATE_COST.
template <bool GATED = false>
__device__ __forceinline__ void pair_box_cost_at(const long p, const int* sel, const int n, const float* __restrict__ det_box,
                                                 const float* __restrict__ trk_box, const int T, const int box_mode, float* __restrict__ box_cost,
                                                 const GateOps& g = GateOps{}) {
    if (T <= 0 || p >= (long)n * T) return;
    const int r = (int)(p / T), t = (int)(p - (long)r * T);
    if (GATED && cross_class(g, sel[r], t)) {
        box_cost[p] = (float)GATE_COST;
        return;
    }
    box_cost[p] = box_pair_cost(*reinterpret_cast<const float4*>(det_box + (long)sel[r] * 4), *reinterpret_cast<const float4*>(trk_box + (long)t * 4), box_mode);
}

// The one store of a pair's re-ID cost (the matrix may sit in mapped host memory and is never read back); GATED: through the motion gate.
template <bool GATED>
__device__ __forceinline__ void put_reid(double* __restrict__ reid_cost, const long p, const double c, const float4 zf, const int t, const GateOps& g) {
    if (GATED && g.kx != nullptr) reid_cost[p] = motion_gated_cost(c, zf, g.kx + (long)t * 8, g.kP + (long)t * 64, g.motion_gate, g.motion_weight);
    else reid_cost[p] = c;
}

// Costs of pair p = r * T + t (kept detection r, track t) of an n x T problem, written at reid_cost[p] / box_cost[p].  GATED: a cross-class pair
// costs GATE_COST in both matrices, and the re-ID cost of the others goes through the motion gate.
template <bool GATED = false>
__device__ __forceinline__ void pair_costs_at(const long p, const int* sel, const int n, const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                              const int E, const float* __restrict__ trk_emb, const float* __restrict__ trk_box, const int T, const int box_mode,
                                              const int reid_metric, double* __restrict__ reid_cost, float* __restrict__ box_cost,
                                              const GateOps& g = GateOps{}) {
    if (T <= 0 || p >= (long)n * T) return;
    const int r = (int)(p / T), t = (int)(p - (long)r * T);
    const int d = sel[r];
    if (GATED && cross_class(g, d, t)) {
        reid_cost[p] = GATE_COST;
        if (box_mode) box_cost[p] = (float)GATE_COST;
        return;
    }
    const float4 zf = GATED && g.kx != nullptr ? *reinterpret_cast<const float4*>(det_box + (long)d * 4) : float4{0.f, 0.f, 0.f, 0.f};
    if (reid_metric == 0) {   // scipy cdist "cosine": 1 - clamp(u.v / (|u| |v|))
        const float* u = det_emb + (long)d * E;
        const float* v = trk_emb + (long)t * E;
        double uu, vv, uv;
        seq_dots(u, v, E, uu, vv, uv);
        double c = uv / (sqrt(uu) * sqrt(vv));
        if (fabs(c) > 1.0) c = copysign(1.0, c);
        put_reid<GATED>(reid_cost, p, (1.0 - c), zf, t, g);
    } else if (reid_metric == 7) {   // scipy cdist "correlation": both rows centred by their float64 mean (numpy's pairwise order), then the cosine kernel
        const float* u = det_emb + (long)d * E;
        const float* v = trk_emb + (long)t * E;
        const double mu = np_pairwise_sum(u, E) / (double)E, mv = np_pairwise_sum(v, E) / (double)E;
        double uu = 0.0, vv = 0.0, uv = 0.0;
        for (int e = 0; e < E; ++e) {
            const double x = (double)u[e] - mu, y = (double)v[e] - mv;
            uu = uu + x * x; vv = vv + y * y; uv = uv + x * y;
        }
        double c = uv / (sqrt(uu) * sqrt(vv));
        if (fabs(c) > 1.0) c = copysign(1.0, c);
        put_reid<GATED>(reid_cost, p, (1.0 - c), zf, t, g);
    } else if (reid_metric <= 2) {   // scipy cdist "euclidean" (1) / "sqeuclidean" (2): s += (u - v)^2 sequentially in float64, then sqrt
        const float* u = det_emb + (long)d * E;
        const float* v = trk_emb + (long)t * E;
        double acc = 0.0;
        for (int e = 0; e < E; ++e) {
            const double df = (double)u[e] - (double)v[e];
            acc = acc + df * df;
        }
        put_reid<GATED>(reid_cost, p, reid_metric == 1 ? sqrt(acc) : acc, zf, t, g);
    } else {                  // "cityblock" (3), "chebyshev" (4), "canberra" (5), "braycurtis" (6): scipy's element order, float64
        const float* u = det_emb + (long)d * E;
        const float* v = trk_emb + (long)t * E;
        double acc = 0.0, den = 0.0;
        for (int e = 0; e < E; ++e) {
            const double x = (double)u[e], y = (double)v[e];
            const double ad = fabs(x - y);
            if (reid_metric == 3) acc = acc + ad;
            else if (reid_metric == 4) acc = ad > acc ? ad : acc;
            else if (reid_metric == 5) {
                const double q = fabs(x) + fabs(y);
                acc = acc + ad / (q + (q == 0.0 ? 1.0 : 0.0));           // 0 / 0 counts as 0
            } else {
                acc = acc + ad;
                den = den + fabs(x + y);
            }
        }
        put_reid<GATED>(reid_cost, p, reid_metric == 6 ? acc / den : acc, zf, t, g);
    }
    if (box_mode)
        box_cost[p] = box_pair_cost(*reinterpret_cast<const float4*>(det_box + (long)d * 4), *reinterpret_cast<const float4*>(trk_box + (long)t * 4), box_mode);
}

// Workgroup blockIdx.x of a 1-D grid of 256-thread workgroups handles pairs 256 * blockIdx.x ... + 255.
__device__ __forceinline__ void pair_costs(const int* sel, const int n, const float* __restrict__ det_emb, const float* __restrict__ det_box, const int E,
                                           const float* __restrict__ trk_emb, const float* __restrict__ trk_box, const int T, const int box_mode,
                                           const int reid_metric, double* __restrict__ reid_cost, float* __restrict__ box_cost) {
    pair_costs_at((long)blockIdx.x * 256 + threadIdx.x, sel, n, det_emb, det_box, E, trk_emb, trk_box, T, box_mode, reid_metric, reid_cost, box_cost);
}

}  // namespace cnl_track
