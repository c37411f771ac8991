// coco_eval.hip — COCO box evaluation (COCOeval, iouType "bbox", no crowds) on the device: the detections stay where the decode left them
// from gather_detection2d to the twelve numbers.  The rule is stated in include/centernet_gfx950.h and restated in numpy in
// tests/coco_eval_ref.py; every float64 operation is rounded on its own, so the two agree bit for bit.
//
//   match_kernel       one workgroup per image, four waves.  Step one ranks the image's detections in LDS (an O(k^2) count): the class
//                      rank of a detection is the number of detections of its label ahead of it (higher score, or the same score and an
//                      earlier slot), and its place in the walk is that plus the detections of smaller labels.  Then wave a serves area
//                      range a and all ten thresholds: it walks the detections in order, the lanes hold the image's ground truths (in
//                      64s), the IoU of a lane is formed once per detection, and per threshold ONE wave maximum over the key
//                      (not ignored, IoU bits) picks the winner — the last lane among equals.  The taken flags of a wave are ten bits
//                      per ground truth in LDS; no wave reads another wave's.
//   accumulate_kernel  one workgroup per (category, area range, maxDet), looping over the thresholds.  The epoch's records arrive ordered
//                      by (label, score descending, arrival).  Pass one counts the segment's true / false positives; pass two walks the
//                      segment's 256-record chunks from the right: a block prefix sum gives tp / fp of every record (the prefix at the
//                      chunk's end is carried leftwards), pr = tp / (fp + tp + eps), a reverse block scan makes it non-increasing from the
//                      right (the maximum is carried leftwards), and the threads r < 101 whose first record with rc >= R[r] lies in the
//                      chunk find it by binary search.  Records of class rank >= maxDet count as neither tp nor fp, like ignored ones:
//                      they repeat their left neighbour's (rc, pr) and are never the FIRST record of an rc value, except before the
//                      first counted record, where the running maximum equals that record's.
// No float atomics; npig is an integer atomic add.  Nothing here synchronises the device.
#include "cnl_common.h"

#pragma clang fp contract(off)   // one rounding per operation (the only fused multiply-adds left are inside the IEEE division sequence)

namespace cnl_coco_eval {

constexpr int THREADS = 256;               // both kernels: four waves
constexpr int WAVES = THREADS / 64;
constexpr int MAX_K = 1024, MAX_G = 1024;  // detections / ground truths per image
constexpr int NT = 10, NA = 4, NM = 3, NR = 101;
constexpr int RANK_CAP = 100;              // maxDets[-1]: the detections of a category kept per image
constexpr unsigned short NO_DET = 0xFFFFu;
constexpr unsigned long long NOT_IGNORED = 1ull << 63;

// np.linspace(.5, .95, 10): the doubles numpy produces (index 8 is one ulp under 0.9), each capped at 1 - 1e-10 as COCOeval does
__device__ __forceinline__ double iou_threshold(int t) {
    constexpr double v[NT] = {0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.8999999999999999, 0.95};
    return v[t] < 1.0 - 1e-10 ? v[t] : 1.0 - 1e-10;
}
__device__ __forceinline__ bool out_of_range(double area, int a) {      // both bounds inclusive: 1024 is small AND medium
    constexpr double lo[NA] = {0.0, 0.0, 1024.0, 9216.0}, hi[NA] = {1e10, 1024.0, 9216.0, 1e10};
    return area < lo[a] || area > hi[a];
}

__host__ __device__ inline int round4(int v) { return (v + 3) & ~3; }
// dynamic LDS of match_kernel: 44 bytes per ground truth + 26 per detection (70 KB at 1024 / 1024, 4.4 KB at 32 / 100)
__host__ __device__ inline size_t match_lds_bytes(int k, int Gmax) { return (size_t)round4(Gmax) * 44 + (size_t)round4(k) * 26; }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {      // in every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(THREADS) void match_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                                                        const long long* __restrict__ labels, const int* __restrict__ count,
                                                        const double* __restrict__ gt_boxes, const long long* __restrict__ gt_labels,
                                                        const int* __restrict__ gt_count, int k, int Gmax, int K, int* __restrict__ out_rank,
                                                        unsigned long long* __restrict__ out_matched, unsigned long long* __restrict__ out_ignored,
                                                        unsigned long long* __restrict__ npig) {
    extern __shared__ double lds[];
    const int Gp = round4(Gmax), kp = round4(k);
    double* const gx = lds;                                   // [Gp] each: the ground truths, xywh
    double* const gy = gx + Gp;
    double* const gw = gy + Gp;
    double* const gh = gw + Gp;
    int* const g_lab = reinterpret_cast<int*>(gh + Gp);       // [Gp]  -1: not a category
    int* const d_lab = g_lab + Gp;                            // [kp]  -1: dropped (past the count, label outside 0..K-1)
    float* const d_score = reinterpret_cast<float*>(d_lab + kp);                         // [kp]
    unsigned short* const order = reinterpret_cast<unsigned short*>(d_score + kp);        // [kp] the walk: (label, class rank) ascending
    unsigned short* const taken = order + kp;                 // [NA][Gp]  bit t: taken at (a, t)
    unsigned short* const d_match = taken + NA * Gp;          // [NA][kp]  bit t
    unsigned short* const d_ign = d_match + NA * kp;          // [NA][kp]

    const int n = blockIdx.x, tid = threadIdx.x;
    const long dbase = (long)n * k, gbase = (long)n * Gmax;
    const int cnt = count ? min(max(count[n], 0), k) : k;
    const int G = min(max(gt_count[n], 0), Gmax);

    for (int d = tid; d < k; d += THREADS) {
        const long long l = labels[dbase + d];
        d_lab[d] = (d < cnt && l >= 0 && l < K) ? (int)l : -1;
        d_score[d] = scores[dbase + d];
        order[d] = NO_DET;
        for (int a = 0; a < NA; ++a) { d_match[a * kp + d] = 0; d_ign[a * kp + d] = 0; }
    }
    for (int g = tid; g < G; g += THREADS) {
        const double* const b = gt_boxes + (gbase + g) * 4;
        const double w = b[2], h = b[3];
        gx[g] = b[0]; gy[g] = b[1]; gw[g] = w; gh[g] = h;
        const long long l = gt_labels[gbase + g];
        const bool is_cat = l >= 0 && l < K;
        g_lab[g] = is_cat ? (int)l : -1;
        for (int a = 0; a < NA; ++a) {
            taken[a * Gp + g] = 0;
            if (is_cat && !out_of_range(w * h, a)) atomicAdd(&npig[l * NA + a], 1ull);
        }
    }
    __syncthreads();

    // class ranks and the walk order
    for (int d = tid; d < k; d += THREADS) {
        const int l = d_lab[d];
        int rank = -1;
        if (l >= 0) {
            const float s = d_score[d];
            int before = 0, ahead = 0;
            for (int e = 0; e < k; ++e) {
                const int le = d_lab[e];
                const float se = d_score[e];
                before += (le >= 0 && le < l);
                ahead += (le == l && (se > s || (se == s && e < d)));
            }
            if (ahead < RANK_CAP) { rank = ahead; order[before + ahead] = (unsigned short)d; }
        }
        out_rank[dbase + d] = rank;
    }
    __syncthreads();

    // wave a: area range a, all thresholds
    const int a = tid >> 6, lane = tid & 63;
    unsigned short* const my_taken = taken + a * Gp;
    for (int p = 0; p < k; ++p) {
        const int d = order[p];                               // uniform
        if (d == NO_DET) continue;
        const float4 b = boxes[dbase + d];
        const int l = d_lab[d];
        const double Dx = (double)b.x, Dy = (double)b.y, Dw = (double)(b.z - b.x), Dh = (double)(b.w - b.y);      // w, h in fp32, then widened
        const double d_area = Dw * Dh;
        unsigned long long best_key[NT];                      // 0: no match yet; else (not ignored) << 63 | IoU bits
        int best_g[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { best_key[t] = 0; best_g[t] = 0; }
        for (int g0 = 0; g0 < G; g0 += 64) {
            const int g = g0 + lane;
            const bool in = g < G && g_lab[g] == l;
            double iou = 0.0;
            unsigned long long key = 0;
            unsigned tk = 0;
            if (in) {
                const double Gx = gx[g], Gy = gy[g], Gw = gw[g], Gh = gh[g];
                const double w = fmin(Dx + Dw, Gx + Gw) - fmax(Dx, Gx);
                const double h = fmin(Dy + Dh, Gy + Gh) - fmax(Dy, Gy);
                if (w > 0.0 && h > 0.0) {
                    const double i = w * h;
                    const double u = (d_area + Gw * Gh) - i;
                    iou = i / u;
                }
                key = (unsigned long long)__double_as_longlong(iou) | (out_of_range(Gw * Gh, a) ? 0ull : NOT_IGNORED);
                tk = my_taken[g];
            }
            if (!__ballot(in && iou >= iou_threshold(0))) continue;        // nothing here reaches the lowest threshold (uniform)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bool elig = in && iou >= iou_threshold(t) && !((tk >> t) & 1u);
                if (!__ballot(elig)) continue;
                const unsigned long long kmax = wave_max_u64(elig ? key : 0ull);
                const unsigned long long win = __ballot(elig && key == kmax);
                if (kmax >= best_key[t]) {                    // a later chunk wins a tie: the last in order
                    best_key[t] = kmax;
                    best_g[t] = g0 + 63 - __clzll((long long)win);
                }
            }
        }
        unsigned m_bits = 0, i_bits = 0;
        const bool det_out = out_of_range(d_area, a);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (best_key[t]) {
                m_bits |= 1u << t;
                if (!(best_key[t] & NOT_IGNORED)) i_bits |= 1u << t;
                if (lane == 0) my_taken[best_g[t]] |= (unsigned short)(1u << t);
            } else if (det_out) {
                i_bits |= 1u << t;
            }
        }
        if (lane == 0) { d_match[a * kp + d] = (unsigned short)m_bits; d_ign[a * kp + d] = (unsigned short)i_bits; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // lane 0's taken flags before the next detection's reads
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();

    for (int d = tid; d < k; d += THREADS) {
        unsigned long long m = 0, ig = 0;
        for (int aa = 0; aa < NA; ++aa) {
            m |= (unsigned long long)d_match[aa * kp + d] << (aa * NT);
            ig |= (unsigned long long)d_ign[aa * kp + d] << (aa * NT);
        }
        out_matched[dbase + d] = m;
        out_ignored[dbase + d] = ig;
    }
}

// inclusive prefix sum over the workgroup, in thread order; `total` in every thread
__device__ __forceinline__ unsigned long long block_scan_add(unsigned long long v, unsigned long long* wave_part, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    if (lane == 63) wave_part[wave] = v;
    __syncthreads();
    unsigned long long add = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const unsigned long long s = wave_part[w];
        if (w < wave) add += s;
        total += s;
    }
    __syncthreads();
    return v + add;
}
// inclusive maximum from the RIGHT over the workgroup (thread i: max of v[i..], and `carry` from the chunks right of this one)
__device__ __forceinline__ double block_rscan_max(double v, double* wave_part, double carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(v, off);
        if (lane + off < 64) v = o > v ? o : v;
    }
    if (lane == 0) wave_part[wave] = v;
    __syncthreads();
    double m = carry;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        const double s = wave_part[w];
        if (w > wave) m = s > m ? s : m;
    }
    __syncthreads();
    return m > v ? m : v;
}

__global__ __launch_bounds__(THREADS) void accumulate_kernel(const int* __restrict__ rank, const unsigned long long* __restrict__ matched,
                                                             const unsigned long long* __restrict__ ignored, const long long* __restrict__ seg,
                                                             const long long* __restrict__ npig, int K, long long total,
                                                             double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ unsigned long long part_sum[WAVES];
    __shared__ double part_max[WAVES];
    __shared__ int s_tp[THREADS];
    __shared__ double s_pr[THREADS];
    const int tid = threadIdx.x;
    const int mi = blockIdx.x % NM, a = (blockIdx.x / NM) % NA, c = blockIdx.x / (NM * NA);
    const int max_det = mi == 0 ? 1 : mi == 1 ? 10 : 100;
    // the category's records: forced inside 0..total whatever the table holds
    const long long s0 = min(max(seg[c], 0ll), total), s1 = min(max(seg[c + 1], s0), total);
    const long long L = s1 - s0;
    const long long np_i = npig[c * NA + a];
    const size_t cell = ((size_t)c * NA + a) * NM + mi, t_stride = (size_t)K * NA * NM;      // precision [T, R, K, A, M], recall [T, K, A, M]
    if (np_i <= 0) {                                         // no ground truth of this category in this range: the cell stays -1
        for (int i = tid; i < NT * NR; i += THREADS) precision[(size_t)i * t_stride + cell] = -1.0;
        if (tid < NT) recall[(size_t)tid * t_stride + cell] = -1.0;
        return;
    }
    const double np_d = (double)np_i;
    const double R = tid < NR ? (tid == NR - 1 ? 1.0 : (double)tid * 0.01) : 2.0;      // np.linspace(0, 1, 101)
    const long long chunks = (L + THREADS - 1) / THREADS;
    for (int t = 0; t < NT; ++t) {
        const int bit = a * NT + t;
        // pass one: the segment's totals
        unsigned long long mine = 0;                         // tp | fp << 32
        for (long long i = s0 + tid; i < s1; i += THREADS) {
            const int r = rank[i];
            if (r >= 0 && r < max_det && !((ignored[i] >> bit) & 1ull)) mine += ((matched[i] >> bit) & 1ull) ? 1ull : (1ull << 32);
        }
        unsigned long long sum;
        block_scan_add(mine, part_sum, sum);
        long long end_tp = (long long)(sum & 0xFFFFFFFFull), end_fp = (long long)(sum >> 32);      // the prefix at the END of the chunk in hand
        if (tid == 0) recall[(size_t)t * t_stride + cell] = L > 0 ? (double)end_tp / np_d : 0.0;
        // pass two: chunks from the right
        double q = 0.0, carry = 0.0;                         // q: this thread's precision entry (0 when rc never reaches R)
        for (long long ch = chunks - 1; ch >= 0; --ch) {
            const long long first = s0 + ch * THREADS, i = first + tid;
            const int n_valid = (int)min((long long)THREADS, s1 - first);
            unsigned long long flag = 0;
            if (i < s1) {
                const int r = rank[i];
                if (r >= 0 && r < max_det && !((ignored[i] >> bit) & 1ull)) flag = ((matched[i] >> bit) & 1ull) ? 1ull : (1ull << 32);
            }
            unsigned long long chunk_sum;
            const unsigned long long incl = block_scan_add(flag, part_sum, chunk_sum);
            const long long start_tp = end_tp - (long long)(chunk_sum & 0xFFFFFFFFull), start_fp = end_fp - (long long)(chunk_sum >> 32);
            const long long tp_i = start_tp + (long long)(incl & 0xFFFFFFFFull), fp_i = start_fp + (long long)(incl >> 32);
            const double tp_d = (double)tp_i;
            const double pr = i < s1 ? tp_d / (((double)fp_i + tp_d) + 0x1p-52) : 0.0;      // np.spacing(1)
            const double pr_max = block_rscan_max(pr, part_max, carry);
            s_tp[tid] = (int)tp_i;
            s_pr[tid] = pr_max;
            __syncthreads();
            carry = s_pr[0];
            // searchsorted(rc, R, "left"): the first record with rc >= R lies here when the chunk's last rc reaches R and the one before the chunk does not
            if (tid < NR && (double)s_tp[n_valid - 1] / np_d >= R && (ch == 0 || !((double)start_tp / np_d >= R))) {
                int lo = 0, hi = n_valid - 1;                // invariant: rc[hi] >= R
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((double)s_tp[mid] / np_d >= R) hi = mid; else lo = mid + 1;
                }
                q = s_pr[lo];
            }
            __syncthreads();
            end_tp = start_tp;
            end_fp = start_fp;
        }
        if (tid < NR) precision[((size_t)t * NR + tid) * t_stride + cell] = q;
    }
}

static cnl::DeviceOnce match_once;

}  // namespace cnl_coco_eval

extern "C" int cnl_coco_match_f64(const float* boxes, const float* scores, const int64_t* labels, const int32_t* count, const double* gt_boxes,
                                  const int64_t* gt_labels, const int32_t* gt_count, int32_t N, int32_t k, int32_t Gmax, int32_t num_classes,
                                  int32_t* out_rank, int64_t* out_matched, int64_t* out_ignored, int64_t* npig, void* stream) {
    using namespace cnl_coco_eval;
    CNL_REQUIRE(N >= 0 && N <= (1 << 20), CNL_E_BAD_ARG, "cnl_coco_match_f64: N = %d outside 0..2^20", N);
    CNL_REQUIRE(k >= 1 && k <= MAX_K, CNL_E_BAD_ARG, "cnl_coco_match_f64: k = %d outside 1..%d", k, MAX_K);
    CNL_REQUIRE(Gmax >= 1 && Gmax <= MAX_G, CNL_E_BAD_ARG, "cnl_coco_match_f64: Gmax = %d outside 1..%d", Gmax, MAX_G);
    CNL_REQUIRE(num_classes >= 1 && num_classes <= (1 << 20), CNL_E_BAD_ARG, "cnl_coco_match_f64: num_classes = %d outside 1..2^20", num_classes);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(boxes && scores && labels && gt_boxes && gt_labels && gt_count && out_rank && out_matched && out_ignored && npig, CNL_E_BAD_ARG,
                "cnl_coco_match_f64: null pointer");
    CNL_REQUIRE(((uintptr_t)boxes & 15) == 0 && (((uintptr_t)labels | (uintptr_t)gt_boxes | (uintptr_t)gt_labels | (uintptr_t)out_matched |
                                                  (uintptr_t)out_ignored | (uintptr_t)npig) & 7) == 0, CNL_E_BAD_ARG,
                "cnl_coco_match_f64: boxes must be 16-byte aligned, the 64-bit arrays 8-byte aligned");
    const size_t lds_bytes = match_lds_bytes(k, Gmax);
    if (int rc = cnl::kernel_setup(match_once, reinterpret_cast<const void*>(match_kernel), (int)match_lds_bytes(MAX_K, MAX_G))) return rc;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)N), dim3(THREADS), lds_bytes, (hipStream_t)stream, reinterpret_cast<const float4*>(boxes), scores,
                       reinterpret_cast<const long long*>(labels), count, gt_boxes, reinterpret_cast<const long long*>(gt_labels), gt_count, k, Gmax,
                       num_classes, out_rank, reinterpret_cast<unsigned long long*>(out_matched), reinterpret_cast<unsigned long long*>(out_ignored),
                       reinterpret_cast<unsigned long long*>(npig));
    return cnl::check_launch("coco_eval match_kernel");
}

extern "C" int cnl_coco_accumulate_f64(const int32_t* rank, const int64_t* matched, const int64_t* ignored, const int64_t* segment_first,
                                       const int64_t* npig, int64_t total, int32_t num_classes, double* precision, double* recall, void* stream) {
    using namespace cnl_coco_eval;
    CNL_REQUIRE(num_classes >= 1 && num_classes <= (1 << 20), CNL_E_BAD_ARG, "cnl_coco_accumulate_f64: num_classes = %d outside 1..2^20", num_classes);
    CNL_REQUIRE(total >= 0 && total < (1ll << 31), CNL_E_BAD_ARG, "cnl_coco_accumulate_f64: total = %lld records outside 0..2^31-1", (long long)total);
    CNL_REQUIRE(segment_first && npig && precision && recall, CNL_E_BAD_ARG, "cnl_coco_accumulate_f64: null pointer");
    CNL_REQUIRE(total == 0 || (rank && matched && ignored), CNL_E_BAD_ARG, "cnl_coco_accumulate_f64: null pointer");
    CNL_REQUIRE((((uintptr_t)matched | (uintptr_t)ignored | (uintptr_t)segment_first | (uintptr_t)npig | (uintptr_t)precision | (uintptr_t)recall) & 7) == 0 &&
                    ((uintptr_t)rank & 3) == 0, CNL_E_BAD_ARG, "cnl_coco_accumulate_f64: the 64-bit arrays must be 8-byte aligned, rank 4-byte aligned");
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)num_classes * NA * NM), dim3(THREADS), 0, (hipStream_t)stream, rank,
                       reinterpret_cast<const unsigned long long*>(matched), reinterpret_cast<const unsigned long long*>(ignored),
                       reinterpret_cast<const long long*>(segment_first), reinterpret_cast<const long long*>(npig), num_classes, (long long)total,
                       precision, recall);
    return cnl::check_launch("coco_eval accumulate_kernel");
}
