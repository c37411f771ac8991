// tile_merge.hip — the merge of sliced inference: the decoded boxes of all views (tiles + the optional full-frame view) of each frame
// go back into the frame's own pixels and the duplicates the tile overlaps create are removed by a class-aware greedy non-maximum
// suppression, for ALL frames of a batch in one launch sequence with no device synchronisation.
//
// The reference imports torchvision.ops.batched_nms (models/centernet.py:10) and never calls it.  The rule here is written so that a
// numpy restatement reproduces it bit for bit (tests/tiled_ref.py): one rounding per operation, a division-free strict
// test inter > t * denom, ties in the score resolved by the candidate number.
//
//   sort_kernel   one workgroup per frame: filter (score > threshold), key = (score descending, candidate number ascending) as ONE
//                 64-bit integer, bitonic sort (in LDS up to SORT_LDS_KEYS keys, in the workspace beyond), cap at max_candidates, then
//                 the sorted candidates' boxes are mapped to the frame and written with label / score / source in sorted order.
//   match_kernel  the suppression bit matrix, row i = the candidates j > i that i would remove: grid = frame x block of 64 rows x group
//                 of 4 column words, the 64 column boxes of a word staged in LDS, one thread per (row, word).  Only words on or right
//                 of the diagonal are computed (match(i, j) is symmetric bit for bit: every operation in it is commutative).
//   walk_kernel   one wave per frame walks the rows in order, 64 at a time: the diagonal words resolve the chunk inside the wave
//                 (v_readlane, no memory), then the rows that survived are OR-ed into the `removed` words right of the chunk with
//                 independent, coalesced loads.  It stops at K_out survivors and writes every output element.
//   soft_kernel   the soft merge (cnl_merge_soft_f32: Gaussian / linear soft-NMS, the multi-scale test) behind the same sort_kernel: one
//                 workgroup per frame runs the whole pick-and-decay loop with every candidate in registers; see the kernel below.
// No float atomics anywhere; a frame's result depends on that frame's views only (its workgroups read nothing else).
#include "cnl_common.h"

#pragma clang fp contract(off)   // one rounding per operation: the restatement in numpy must agree bit for bit

namespace cnl_tile_merge {

constexpr int SORT_THREADS = 512;
constexpr int SORT_LDS_KEYS = 4096;        // 32 KB of LDS; a frame of 16 views x 100 detections pads to 2048 keys
constexpr int MATCH_WORDS = 4;             // column words per match workgroup (256 threads = 64 rows x 4 words)
constexpr int MAX_CANDIDATES = 16384;      // 256 row words: walk_kernel keeps the `removed` words of a frame in 2 KB of LDS
constexpr unsigned long long INVALID_KEY = ~0ull;

struct View {                              // one record of `views` (32 bytes; include/centernet_gfx950.h)
    int frame_w, frame_h, x0, y0, pad_left, pad_top;
    float sx, sy;
};
struct FrameHead {                         // written by sort_kernel, read by the other two (16 bytes per frame)
    int M;                                 // candidates that take part: min(survivors of the threshold, max_candidates)
    int reserved;
    unsigned long long matrix_offset;      // first word of the frame's bit matrix
};

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// workspace carve-up; T = V * k candidates in all
struct Layout {
    size_t head, keys, box, label, source, score, matrix, total;
    // with_matrix = false: the soft merge, which has no suppression bit matrix (`matrix` is then an empty tail)
    __host__ Layout(int N, int V, int k, int max_candidates, bool with_matrix = true) {
        const size_t T = (size_t)V * k;
        const size_t rows = T < (size_t)N * max_candidates ? T : (size_t)N * max_candidates;      // sum over frames of min(C_n, max_candidates)
        size_t o = 0;
        head = o;   o = align256(o + (size_t)N * sizeof(FrameHead));
        keys = o;   o = align256(o + 2 * T * 8);                      // a frame's keys padded to a power of two: < 2 C_n
        box = o;    o = align256(o + T * 16);
        label = o;  o = align256(o + T * 4);
        source = o; o = align256(o + T * 4);
        score = o;  o = align256(o + T * 4);
        matrix = o; o = align256(o + (with_matrix ? rows * (size_t)((max_candidates + 63) / 64) * 8 : 0));
        total = o;
    }
};

__device__ __forceinline__ int row_words(int M) { return (M + 63) >> 6; }
// the views [v0, v1) of frame n, forced inside 0..V whatever the table holds: every index below derives from them
__device__ __forceinline__ void frame_views(const int* __restrict__ first_view, int n, int V, int& v0, int& v1) {
    v0 = min(max(first_view[n], 0), V);
    v1 = min(max(first_view[n + 1], v0), V);
}

__global__ __launch_bounds__(SORT_THREADS) void sort_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                                                            const long long* __restrict__ labels, const View* __restrict__ views,
                                                            const int* __restrict__ first_view, int V, int k, int max_candidates, float score_threshold,
                                                            unsigned long long matrix_words, FrameHead* __restrict__ head, unsigned long long* __restrict__ ws_keys,
                                                            float4* __restrict__ s_box, int* __restrict__ s_label, int* __restrict__ s_source,
                                                            float* __restrict__ s_score) {
    __shared__ unsigned long long lds_keys[SORT_LDS_KEYS];
    __shared__ int n_valid;
    __shared__ unsigned long long offset;
    const int n = blockIdx.x, tid = threadIdx.x;
    int v0, v1;
    frame_views(first_view, n, V, v0, v1);
    const long base = (long)v0 * k;                         // the frame's first candidate
    const int C = (v1 - v0) * k;
    int P = 1;
    while (P < C) P <<= 1;
    unsigned long long* const keys = P <= SORT_LDS_KEYS ? lds_keys : ws_keys + 2 * base;
    if (tid == 0) { n_valid = 0; offset = 0; }
    __syncthreads();

    // where this frame's bit matrix starts: the frames before it take min(C_m, max_candidates) rows of that many bits, rounded up to words
    unsigned long long before = 0;
    for (int m = tid; m < n; m += SORT_THREADS) {
        int m0, m1;
        frame_views(first_view, m, V, m0, m1);
        const int Mb = min((m1 - m0) * k, max_candidates);
        before += (unsigned long long)Mb * (unsigned long long)row_words(Mb);
    }
    if (before) atomicAdd(&offset, before);

    int mine = 0;
    for (int c = tid; c < P; c += SORT_THREADS) {
        unsigned long long key = INVALID_KEY;
        if (c < C) {
            const float s = scores[base + c];
            if (s > score_threshold) {                      // false for NaN
                unsigned u = __float_as_uint(s + 0.0f);     // -0 -> +0: equal scores must have equal keys
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // monotone in the float order
                key = ((unsigned long long)(~u) << 32) | (unsigned)c;
                ++mine;
            }
        }
        keys[c] = key;
    }
    if (mine) atomicAdd(&n_valid, mine);
    __syncthreads();

    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += SORT_THREADS) {
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo | stride;
                const unsigned long long a = keys[lo], b = keys[hi];
                const bool up = (lo & size) == 0;
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    }

    int M = min(n_valid, max_candidates);
    // (a table whose frames share views could ask for more matrix than the workspace has: such a frame merges nothing)
    if (offset + (unsigned long long)min(C, max_candidates) * (unsigned long long)row_words(min(C, max_candidates)) > matrix_words) M = 0;
    if (tid == 0) {
        FrameHead h;
        h.M = M; h.reserved = 0; h.matrix_offset = offset;
        head[n] = h;
    }
    for (int i = tid; i < M; i += SORT_THREADS) {
        const unsigned c = (unsigned)keys[i];
        const View vw = views[v0 + (int)(c / (unsigned)k)];
        float4 b = boxes[base + c];
        const float pl = (float)vw.pad_left, pt = (float)vw.pad_top, ox = (float)vw.x0, oy = (float)vw.y0;
        const float wf = (float)vw.frame_w, hf = (float)vw.frame_h;
        b.x = fminf(fmaxf((b.x - pl) / vw.sx + ox, 0.f), wf);
        b.y = fminf(fmaxf((b.y - pt) / vw.sy + oy, 0.f), hf);
        b.z = fminf(fmaxf((b.z - pl) / vw.sx + ox, 0.f), wf);
        b.w = fminf(fmaxf((b.w - pt) / vw.sy + oy, 0.f), hf);
        s_box[base + i] = b;
        s_label[base + i] = (int)labels[base + c];
        s_source[base + i] = (int)c;
        s_score[base + i] = scores[base + c];
    }
}

__device__ __forceinline__ bool match(const float4 a, const float area_a, const float4 b, float t, int ios) {
    const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = iw * ih;
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float denom = ios ? fminf(area_a, area_b) : (area_a + area_b) - inter;
    return inter > t * denom;
}

__global__ __launch_bounds__(64 * MATCH_WORDS) void match_kernel(const FrameHead* __restrict__ head, const int* __restrict__ first_view, int V, int k,
                                                                 const float4* __restrict__ s_box, const int* __restrict__ s_label,
                                                                 float match_threshold, int ios, int class_aware,
                                                                 unsigned long long* __restrict__ matrix) {
    __shared__ float4 cbox[MATCH_WORDS][64];
    __shared__ int clabel[MATCH_WORDS][64];
    const int n = blockIdx.z, rb = blockIdx.y, wg = blockIdx.x;
    const FrameHead h = head[n];
    const int M = h.M, W = row_words(M);
    // uniform exits: rows past the frame's candidates, word groups wholly left of the diagonal or past the last word
    if (rb * 64 >= M || wg * MATCH_WORDS >= W || wg * MATCH_WORDS + MATCH_WORDS - 1 < rb) return;
    const long base = (long)min(max(first_view[n], 0), V) * k;
    const int lane = threadIdx.x & 63, ww = threadIdx.x >> 6, w = wg * MATCH_WORDS + ww;
    {
        const int j = w * 64 + lane;
        const bool in = w < W && j < M;
        cbox[ww][lane] = in ? s_box[base + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        clabel[ww][lane] = in ? s_label[base + j] : -1;
    }
    __syncthreads();
    const int i = rb * 64 + lane;
    if (i >= M || w >= W || w < rb) return;
    const float4 a = s_box[base + i];
    const int la = s_label[base + i];
    const float area_a = (a.z - a.x) * (a.w - a.y);
    unsigned long long bits = 0;
    const int j_end = min(64, M - w * 64);
    for (int jj = 0; jj < j_end; ++jj) {
        const bool m = (w * 64 + jj > i) && (!class_aware || clabel[ww][jj] == la) && match(a, area_a, cbox[ww][jj], match_threshold, ios);
        bits |= (unsigned long long)m << jj;
    }
    matrix[h.matrix_offset + (unsigned long long)i * W + w] = bits;
}

__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v, int lane) {      // `lane` is uniform
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void walk_kernel(const FrameHead* __restrict__ head, const int* __restrict__ first_view, int V, int k, int K_out,
                                                  const float4* __restrict__ s_box, const int* __restrict__ s_label,
                                                  const int* __restrict__ s_source, const float* __restrict__ s_score,
                                                  const unsigned long long* __restrict__ matrix, float4* __restrict__ out_boxes,
                                                  float* __restrict__ out_scores, long long* __restrict__ out_labels,
                                                  int* __restrict__ out_source, int* __restrict__ out_count) {
    __shared__ unsigned long long removed[MAX_CANDIDATES / 64];
    const int n = blockIdx.x, lane = threadIdx.x;
    const FrameHead h = head[n];
    const int M = h.M, W = row_words(M);
    const long base = (long)min(max(first_view[n], 0), V) * k;
    const unsigned long long* const rows = matrix + h.matrix_offset;
    for (int w = lane; w < W; w += 64) removed[w] = 0;
    __syncthreads();
    int kept = 0;                                            // uniform
    for (int b = 0; b < W && kept < K_out; ++b) {
        const int i = b * 64 + lane;
        const unsigned long long diag = i < M ? rows[(unsigned long long)i * W + b] : 0ull;
        unsigned long long rem = removed[b], keep = 0;       // both uniform
        const int t_end = min(64, M - b * 64);
        int kept_here = 0;
        for (int t = 0; t < t_end && kept + kept_here < K_out; ++t) {
            const unsigned long long row = read_lane64(diag, t);
            if (!((rem >> t) & 1ull)) {
                keep |= 1ull << t;
                rem |= row;
                ++kept_here;
            }
        }
        if ((keep >> lane) & 1ull) {
            const long o = (long)n * K_out + kept + __popcll(keep & ((1ull << lane) - 1ull));
            out_boxes[o] = s_box[base + i];
            out_scores[o] = s_score[base + i];
            out_labels[o] = (long long)s_label[base + i];
            out_source[o] = s_source[base + i];
        }
        kept += kept_here;
        if (kept >= K_out) break;
        // the rows that survived remove candidates right of this chunk: one word column per lane, the rows' loads independent
        for (int w = b + 1 + lane; w < W; w += 64) {
            unsigned long long acc = removed[w];
            for (unsigned long long left = keep; left; left &= left - 1) {
                const int t = __ffsll((long long)left) - 1;
                acc |= rows[(unsigned long long)(b * 64 + t) * W + w];
            }
            removed[w] = acc;
        }
        __syncthreads();
    }
    for (int r = kept + lane; r < K_out; r += 64) {
        const long o = (long)n * K_out + r;
        out_boxes[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        out_scores[o] = 0.f;
        out_labels[o] = 0;
        out_source[o] = -1;
    }
    if (lane == 0) out_count[n] = kept;
}

// ---------------------------------------------------------------------------------------------------------------- the soft merge
// soft_kernel: soft-NMS (Bodla et al.) behind the same sort stage, the rule of include/centernet_gfx950.h (cnl_merge_soft_f32).  A kept
// box lowers its neighbours' scores, which changes who is picked next: nothing a bit matrix can hold, so the kernel IS the loop.
// One workgroup of 256 threads per frame.  Position p (the index in the sorted order) belongs to thread p % 256, slot p / 256: a
// thread keeps the box, label, source and float64 working score of its <= 16 candidates in registers (every index below is a constant
// of an unrolled loop) and, beside them, its best live candidate.  A pick is: wave maximum of (score, position) by 6 xor-shuffles,
// the owning lane of each wave publishes its candidate whole (48 bytes) in LDS, one barrier, every thread reads the 4 entries and knows
// the winner and its box; then each thread decays its same-label candidates and finds its new best in the same pass.  The LDS entries
// alternate between two buffers, so that one barrier per pick is enough.  The trip count is uniform: the winner is read by all
// threads from the same LDS words.
constexpr int SOFT_THREADS = 256;
constexpr int SOFT_SLOTS = 16;
constexpr int SOFT_MAX_CANDIDATES = SOFT_THREADS * SOFT_SLOTS;      // 4096: nine scales x 300 detections fit
constexpr int SOFT_WAVES = SOFT_THREADS / 64;
constexpr int NO_POSITION = 0x7fffffff;

struct alignas(16) SoftBest {              // what a wave publishes per pick (48 bytes)
    double score;
    int position, label, source, reserved;
    float4 box;
};

__device__ __forceinline__ double neg_inf() { return -__builtin_inf(); }

// the weight the pick `a` puts on candidate `b` (rule 5 of cnl_merge_soft_f32); METHOD 0 is the fp32 predicate of the hard merge itself
template <int METHOD>
__device__ __forceinline__ double soft_weight(const float4 a, const float area_a, const float4 b, const float t, const double td, const double sigma) {
    if (METHOD == 0) return match(a, area_a, b, t, 0) ? 0.0 : 1.0;
    const double ax = a.x, ay = a.y, az = a.z, aw = a.w, bx = b.x, by = b.y, bz = b.z, bw = b.w;
    const double iw = fmax(fmin(az, bz) - fmax(ax, bx), 0.0), ih = fmax(fmin(aw, bw) - fmax(ay, by), 0.0);
    const double inter = iw * ih;
    if (!(inter > 0.0)) return 1.0;        // ov = 0 (or ua is not positive): exp(-0) = 1 and 1 - 0 = 1 exactly, so nothing is skipped but work
    const double ua = ((az - ax) * (aw - ay) + (bz - bx) * (bw - by)) - inter;
    if (!(ua > 0.0)) return 1.0;
    const double ov = inter / ua;
    if (METHOD == 2) return exp(-(ov * ov) / sigma);
    return ov > td ? 1.0 - ov : 1.0;
}

template <int METHOD>
__global__ __launch_bounds__(SOFT_THREADS) void soft_kernel(const FrameHead* __restrict__ head, const int* __restrict__ first_view, int V, int k, int K_out,
                                                            const float4* __restrict__ s_box, const int* __restrict__ s_label,
                                                            const int* __restrict__ s_source, const float* __restrict__ s_score,
                                                            float score_threshold, float sigma_f, float iou_threshold, int class_aware,
                                                            float4* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                            long long* __restrict__ out_labels, int* __restrict__ out_source,
                                                            int* __restrict__ out_count) {
    __shared__ SoftBest published[2][SOFT_WAVES];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = min(max(head[n].M, 0), SOFT_MAX_CANDIDATES);          // (the entry point has bounded max_candidates: the clamp costs nothing)
    const int S = (M + SOFT_THREADS - 1) / SOFT_THREADS;                // slots in use, uniform
    const long base = (long)min(max(first_view[n], 0), V) * k;
    const double thr = score_threshold, sigma = sigma_f, td = iou_threshold;

    float4 box[SOFT_SLOTS];
    int label[SOFT_SLOTS], source[SOFT_SLOTS];
    double work[SOFT_SLOTS];               // the working score; -inf: picked, or no candidate in the slot
    double best_s = neg_inf();             // this thread's best live candidate, carried whole
    int best_p = NO_POSITION, best_label = 0, best_source = -1;
    float4 best_box = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < SOFT_SLOTS; ++s) {
        const int p = s * SOFT_THREADS + tid;
        const bool in = p < M;
        box[s] = in ? s_box[base + p] : make_float4(0.f, 0.f, 0.f, 0.f);
        label[s] = in ? s_label[base + p] : 0;
        source[s] = in ? s_source[base + p] : -1;
        work[s] = in ? (double)s_score[base + p] : neg_inf();
        if (work[s] > thr && work[s] > best_s) {                        // (slots ascend: an equal score later loses to the lower position)
            best_s = work[s]; best_p = p; best_label = label[s]; best_source = source[s]; best_box = box[s];
        }
    }

    int r = 0;                                                          // uniform
    for (; r < K_out; ++r) {
        // the wave's maximum: larger score, then lower position
        double ws = best_s;
        int wp = best_p;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(ws, off);
            const int op = __shfl_xor(wp, off);
            if (os > ws || (os == ws && op < wp)) { ws = os; wp = op; }
        }
        SoftBest* const slot = &published[r & 1][wave];
        if (wp == NO_POSITION ? lane == 0 : wp == best_p) {             // positions are unique: exactly one lane of the wave
            SoftBest e;
            e.score = ws; e.position = wp; e.label = best_label; e.source = best_source; e.reserved = 0; e.box = best_box;
            *slot = e;
        }
        __syncthreads();
        int win = 0;
        double pick_s = published[r & 1][0].score;
        int pick_p = published[r & 1][0].position;
#pragma unroll
        for (int w = 1; w < SOFT_WAVES; ++w) {
            const double os = published[r & 1][w].score;
            const int op = published[r & 1][w].position;
            if (os > pick_s || (os == pick_s && op < pick_p)) { pick_s = os; pick_p = op; win = w; }
        }
        if (pick_p == NO_POSITION) break;                               // no live candidate is left
        const SoftBest pick = published[r & 1][win];
        if (tid == 0) {
            const long o = (long)n * K_out + r;
            out_boxes[o] = pick.box;
            out_scores[o] = (float)pick_s;
            out_labels[o] = (long long)pick.label;
            out_source[o] = pick.source;
        }
        if (r + 1 == K_out) { ++r; break; }
        // decay, and the new local best, in one pass
        const float area_pick = (pick.box.z - pick.box.x) * (pick.box.w - pick.box.y);
        best_s = neg_inf();
        best_p = NO_POSITION;
#pragma unroll
        for (int s = 0; s < SOFT_SLOTS; ++s) {
            if (s < S) {
                const int p = s * SOFT_THREADS + tid;
                double v = work[s];
                if (p == pick_p) v = neg_inf();
                else if (v > neg_inf() && (!class_aware || label[s] == pick.label))
                    v = v * soft_weight<METHOD>(pick.box, area_pick, box[s], iou_threshold, td, sigma);
                work[s] = v;
                if (v > thr && v > best_s) { best_s = v; best_p = p; best_label = label[s]; best_source = source[s]; best_box = box[s]; }
            }
        }
    }
    for (int q = r + tid; q < K_out; q += SOFT_THREADS) {
        const long o = (long)n * K_out + q;
        out_boxes[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        out_scores[o] = 0.f;
        out_labels[o] = 0;
        out_source[o] = -1;
    }
    if (tid == 0) out_count[n] = r;
}

// What the two merges share on the host.  `limit` is the entry point's own bound on max_candidates: where it is tighter than the common
// one (the soft merge's) it is reported first; the workspace queries have no K_out.
static int merge_check_sizes(const char* who, int32_t N, int32_t V, int32_t k, int32_t max_candidates, int limit = MAX_CANDIDATES, int32_t K_out = 1) {
    const bool within = max_candidates >= 1 && max_candidates <= limit;
    if (limit < MAX_CANDIDATES) CNL_REQUIRE(within, CNL_E_BAD_ARG, "%s: max_candidates = %d outside 1..%d", who, max_candidates, limit);
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "%s: N = %d outside 0..65535", who, N);
    CNL_REQUIRE(V >= 0 && k >= 1, CNL_E_BAD_ARG, "%s: V = %d must be >= 0 and k = %d >= 1", who, V, k);
    CNL_REQUIRE((long)V * k <= (1L << 30), CNL_E_BAD_ARG, "%s: V * k = %ld candidates exceed 2^30", who, (long)V * k);
    CNL_REQUIRE(within, CNL_E_BAD_ARG, "%s: max_candidates = %d outside 1..%d", who, max_candidates, limit);
    CNL_REQUIRE(K_out >= 1, CNL_E_BAD_ARG, "%s: K_out = %d must be at least 1", who, K_out);
    return CNL_OK;
}

struct MergeCall {                         // the workspace carved up (Layout) and the stream: what an entry point's own kernels are launched with
    FrameHead* head;
    float4* s_box;
    int* s_label;
    int* s_source;
    float* s_score;
    unsigned long long* matrix;            // (an empty tail without with_matrix)
    hipStream_t stream;
};

// after an entry point's own checks, for N >= 1: the pointer and workspace checks, the carve-up, and the sort stage both merges start with
static int merge_begin(const char* who, bool with_matrix, const float* boxes, const float* scores, const int64_t* labels, const void* views,
                       const int32_t* frame_first_view, int32_t N, int32_t V, int32_t k, int32_t max_candidates, float score_threshold,
                       const float* out_boxes, const float* out_scores, const int64_t* out_labels, const int32_t* out_source, const int32_t* out_count,
                       void* ws, size_t ws_bytes, void* stream, MergeCall& c) {
    CNL_REQUIRE(frame_first_view && out_boxes && out_scores && out_labels && out_source && out_count, CNL_E_BAD_ARG, "%s: null pointer", who);
    CNL_REQUIRE(V == 0 || (boxes && scores && labels && views), CNL_E_BAD_ARG, "%s: null pointer", who);
    CNL_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)out_boxes & 15) == 0 && ((uintptr_t)views & 3) == 0 && ((uintptr_t)labels & 7) == 0 &&
                    ((uintptr_t)out_labels & 7) == 0, CNL_E_BAD_ARG,
                "%s: boxes and out_boxes must be 16-byte, labels and out_labels 8-byte, views 4-byte aligned", who);
    const Layout L(N, V, k, max_candidates, with_matrix);
    CNL_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, CNL_E_WORKSPACE, "%s: the workspace must be 256-byte aligned and not null", who);
    CNL_REQUIRE(ws_bytes >= L.total, CNL_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
    char* const w = static_cast<char*>(ws);
    c = MergeCall{reinterpret_cast<FrameHead*>(w + L.head), reinterpret_cast<float4*>(w + L.box), reinterpret_cast<int*>(w + L.label),
                  reinterpret_cast<int*>(w + L.source), reinterpret_cast<float*>(w + L.score), reinterpret_cast<unsigned long long*>(w + L.matrix),
                  (hipStream_t)stream};
    // the sort stage's "does the matrix fit" test: the words the workspace has for it, or no limit where there is no bit matrix
    const unsigned long long matrix_words = with_matrix ? (unsigned long long)((L.total - L.matrix) / 8) : ~0ull;
    hipLaunchKernelGGL(sort_kernel, dim3((unsigned)N), dim3(SORT_THREADS), 0, c.stream, reinterpret_cast<const float4*>(boxes), scores,
                       reinterpret_cast<const long long*>(labels), static_cast<const View*>(views), frame_first_view, V, k, max_candidates,
                       score_threshold, matrix_words, c.head, reinterpret_cast<unsigned long long*>(w + L.keys), c.s_box, c.s_label, c.s_source, c.s_score);
    return cnl::check_launch("tile_merge sort_kernel");
}

}  // namespace cnl_tile_merge

extern "C" size_t cnl_merge_tiles_workspace_bytes(int32_t N, int32_t V, int32_t k, int32_t max_candidates) {
    if (cnl_tile_merge::merge_check_sizes("cnl_merge_tiles_workspace_bytes", N, V, k, max_candidates) != CNL_OK) return 0;
    return cnl_tile_merge::Layout(N, V, k, max_candidates).total;
}

extern "C" int cnl_merge_tiles_f32(const float* boxes, const float* scores, const int64_t* labels, const void* views,
                                   const int32_t* frame_first_view, int32_t N, int32_t V, int32_t k, int32_t K_out, int32_t max_candidates,
                                   float score_threshold, float match_threshold, int32_t metric, int32_t class_aware, float* out_boxes,
                                   float* out_scores, int64_t* out_labels, int32_t* out_source, int32_t* out_count, void* ws, size_t ws_bytes,
                                   void* stream) {
    using namespace cnl_tile_merge;
    if (int rc = merge_check_sizes("cnl_merge_tiles_f32", N, V, k, max_candidates, MAX_CANDIDATES, K_out)) return rc;
    CNL_REQUIRE(metric == 0 || metric == 1, CNL_E_BAD_ARG, "cnl_merge_tiles_f32: metric = %d is neither 0 (IoU) nor 1 (IoS)", metric);
    CNL_REQUIRE(score_threshold == score_threshold && match_threshold == match_threshold, CNL_E_BAD_ARG, "cnl_merge_tiles_f32: a threshold is NaN");
    if (N == 0) return CNL_OK;
    MergeCall c;
    if (int rc = merge_begin("cnl_merge_tiles_f32", true, boxes, scores, labels, views, frame_first_view, N, V, k, max_candidates, score_threshold,
                             out_boxes, out_scores, out_labels, out_source, out_count, ws, ws_bytes, stream, c)) return rc;
    // no frame has more candidates than all of them: the grid covers min(V * k, max_candidates) rows, workgroups past a frame's own M leave at once
    const long rows_max = (long)V * k < max_candidates ? (long)V * k : max_candidates;
    if (rows_max > 0) {
        const unsigned row_blocks = (unsigned)((rows_max + 63) / 64);
        hipLaunchKernelGGL(match_kernel, dim3((row_blocks + MATCH_WORDS - 1) / MATCH_WORDS, row_blocks, (unsigned)N), dim3(64 * MATCH_WORDS), 0, c.stream,
                           c.head, frame_first_view, V, k, c.s_box, c.s_label, match_threshold, metric, class_aware, c.matrix);
        if (int rc = cnl::check_launch("tile_merge match_kernel")) return rc;
    }
    hipLaunchKernelGGL(walk_kernel, dim3((unsigned)N), dim3(64), 0, c.stream, c.head, frame_first_view, V, k, K_out, c.s_box, c.s_label, c.s_source,
                       c.s_score, c.matrix, reinterpret_cast<float4*>(out_boxes), out_scores, reinterpret_cast<long long*>(out_labels), out_source, out_count);
    return cnl::check_launch("tile_merge walk_kernel");
}

extern "C" size_t cnl_merge_soft_workspace_bytes(int32_t N, int32_t V, int32_t k, int32_t max_candidates) {
    using namespace cnl_tile_merge;
    if (merge_check_sizes("cnl_merge_soft_workspace_bytes", N, V, k, max_candidates, SOFT_MAX_CANDIDATES) != CNL_OK) return 0;
    return Layout(N, V, k, max_candidates, false).total;
}

extern "C" int cnl_merge_soft_f32(const float* boxes, const float* scores, const int64_t* labels, const void* views,
                                  const int32_t* frame_first_view, int32_t N, int32_t V, int32_t k, int32_t K_out, int32_t max_candidates,
                                  float score_threshold, int32_t method, float sigma, float iou_threshold, int32_t class_aware, float* out_boxes,
                                  float* out_scores, int64_t* out_labels, int32_t* out_source, int32_t* out_count, void* ws, size_t ws_bytes,
                                  void* stream) {
    using namespace cnl_tile_merge;
    if (int rc = merge_check_sizes("cnl_merge_soft_f32", N, V, k, max_candidates, SOFT_MAX_CANDIDATES, K_out)) return rc;
    CNL_REQUIRE(method >= 0 && method <= 2, CNL_E_BAD_ARG, "cnl_merge_soft_f32: method = %d is none of 0 (hard), 1 (linear), 2 (gaussian)", method);
    CNL_REQUIRE(score_threshold == score_threshold && iou_threshold == iou_threshold, CNL_E_BAD_ARG, "cnl_merge_soft_f32: a threshold is NaN");
    CNL_REQUIRE(sigma > 0.f && sigma <= 3.402823466e38f, CNL_E_BAD_ARG, "cnl_merge_soft_f32: sigma = %g must be positive and finite", (double)sigma);
    if (N == 0) return CNL_OK;
    MergeCall c;
    if (int rc = merge_begin("cnl_merge_soft_f32", false, boxes, scores, labels, views, frame_first_view, N, V, k, max_candidates, score_threshold,
                             out_boxes, out_scores, out_labels, out_source, out_count, ws, ws_bytes, stream, c)) return rc;
    auto* const kernel = method == 0 ? soft_kernel<0> : method == 1 ? soft_kernel<1> : soft_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)N), dim3(SOFT_THREADS), 0, c.stream, c.head, frame_first_view, V, k, K_out, c.s_box, c.s_label, c.s_source,
                       c.s_score, score_threshold, sigma, iou_threshold, class_aware, reinterpret_cast<float4*>(out_boxes), out_scores,
                       reinterpret_cast<long long*>(out_labels), out_source, out_count);
    return cnl::check_launch("tile_merge soft_kernel");
}
