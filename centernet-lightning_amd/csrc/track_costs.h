// track_costs.h — the device code that turns one frame's detections into association costs: the detection-threshold compaction and the
// per-pair re-ID (float64) / box (float32) costs.  Shared by track.hip (one stream per launch) and track_streams.hip (S streams per
// launch) so that both write bit-identical matrices: the integer decisions taken from them (thresholds, assignment) must not depend on
// which entry point computed them.
#pragma once
#include "cnl_common.h"

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

// Box costs alone of pair p = r * T + t of an n x T problem (the low-score stage: no re-ID matrix), written at box_cost[p].
__device__ __forceinline__ void pair_box_cost_at(const long p, const int* sel, const int n, const float* __restrict__ det_box,
                                                 const float* __restrict__ trk_box, const int T, const int box_mode, float* __restrict__ box_cost) {
    if (T <= 0 || p >= (long)n * T) return;
    const int r = (int)(p / T), t = (int)(p - (long)r * T);
    box_cost[p] = box_pair_cost(*reinterpret_cast<const float4*>(det_box + (long)sel[r] * 4), *reinterpret_cast<const float4*>(trk_box + (long)t * 4), box_mode);
}

// Costs of pair p = r * T + t (kept detection r, track t) of an n x T problem, written at reid_cost[p] / box_cost[p].
__device__ __forceinline__ void pair_costs_at(const long p, const int* sel, const int n, const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                              const int E, const float* __restrict__ trk_emb, const float* __restrict__ trk_box, const int T, const int box_mode,
                                              const int reid_metric, double* __restrict__ reid_cost, float* __restrict__ box_cost) {
    if (T <= 0 || p >= (long)n * T) return;
    const int r = (int)(p / T), t = (int)(p - (long)r * T);
    const int d = sel[r];
    if (reid_metric == 0) {   // scipy cdist "cosine": 1 - clamp(u.v / (|u| |v|))
        const float* u = det_emb + (long)d * E;
        const float* v = trk_emb + (long)t * E;
        double uu, vv, uv;
        seq_dots(u, v, E, uu, vv, uv);
        double c = uv / (sqrt(uu) * sqrt(vv));
        if (fabs(c) > 1.0) c = copysign(1.0, c);
        reid_cost[p] = (1.0 - c);
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
        reid_cost[p] = (1.0 - c);
    } else if (reid_metric <= 2) {   // scipy cdist "euclidean" (1) / "sqeuclidean" (2): s += (u - v)^2 sequentially in float64, then sqrt
        const float* u = det_emb + (long)d * E;
        const float* v = trk_emb + (long)t * E;
        double acc = 0.0;
        for (int e = 0; e < E; ++e) {
            const double df = (double)u[e] - (double)v[e];
            acc = acc + df * df;
        }
        reid_cost[p] = reid_metric == 1 ? sqrt(acc) : acc;
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
        reid_cost[p] = reid_metric == 6 ? acc / den : acc;
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
