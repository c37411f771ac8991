// reid_loss.hip — the re-ID (track identity) loss of the tracking model (reference models/fairmot.py:34-61 EmbeddingHead.compute_loss: gather at the
// box centres, Linear(D, D) / BatchNorm1d / ReLU / Linear(D, K), cross entropy over K identities) and its analytic gradient, float64 on the fp32
// values, in fixed summation orders: no atomics, no memset, the same bits on every run.  The rule is stated in include/centernet_gfx950.h and
// restated in numpy in tests/reid_loss_ref.py.  The R x K logits (R = N Gmax rows) are never written to memory.
//
//   row_kernel       one thread per slot (n, g): state (0 none, 1 statistics only, 2 live), cell, identity; per_row <- 0 where the row is not live.
//   count_kernel     one workgroup: the stat rows and the live rows compacted in (n, g) order (ballot + popcount prefix), the counts; a training call
//                    with fewer than two stat rows empties both lists (value 0, gradients 0, running statistics kept).
//   gather_kernel    E[r, :] <- the D fp32 values at the row's cell, widened.          hidden_kernel   H[r, j] = sum_i W1[j, i] E[r, i], i ascending.
//   bn_stats_kernel  a workgroup per 16 features: mean and biased variance over the stat rows in list order (128-row tiles through LDS, one thread
//                    per feature adds them in order); the running statistics after the step.
//   act_kernel       Z[r, j] = max(0, (H - mean) / sd * gamma + beta) of the live rows.
//   ce_kernel        the hot path.  A workgroup owns 32 live rows; W2 streams through LDS in tiles of 64 identities x 32 features, converted to float64
//                    at staging; a thread holds 2 rows x 4 identities of logits in registers (fused multiply-add, j ascending); the 16 lanes that hold a
//                    row's 64 logits fold the tile's maximum, arg-maximum and sum of exponentials with a butterfly and keep a running (max, sum).
//   finish_kernel    one workgroup: sum of ce over the live rows in order / (M + 1e-8), top-1 hits, the counts.
// Gradient (second half): ce_kernel again for lse, then
//   dz_kernel        by row block: logits recomputed, g = scale (softmax - onehot) / (M + 1e-8) through LDS, dZ[r, j] += sum_k g[r, k] W2[k, j], k ascending.
//   dw2_kernel       by identity tile, walking all live rows in order: dW2[k, j] = sum_r g[r, k] Z[r, j], db2[k] = sum_r g[r, k]; stored once.
//   bn_grad_kernel   dbeta, dgamma and the two sums of the BatchNorm backward, over the live rows in order.      dh_kernel   dH of every stat row.
//   dw1_kernel       a workgroup per 16 x 16 tile of dW1 = sum_r dH[r, j] E[r, i], stat rows in order.           de_kernel   dE[r, i] = sum_j W1[j, i] dH[r, j].
//   scatter_kernel   a workgroup owns a tile of one image over all D channels (loss_common.h: Tile, element): the image's stat rows whose cell lies in
//                    the tile are staged in LDS in slot order (stage_pass); every element is stored exactly once: the sum of its rows' dE in slot order, or 0.
// Nothing here synchronises the device.
#include "loss_common.h"

#pragma clang fp contract(off)   // one rounding per operation; the products' accumulation is an explicit fma()

namespace cnl_reid_loss {

using namespace cnl_loss;

constexpr int MAX_D = 256, MAX_K = 1 << 20;
constexpr int RB = 32, KT = 64, DC = 32;           // rows per block, identities per tile, features per staged chunk
constexpr int ZS_LD = RB + 2, WS_LD = KT + 2;      // LDS row pitches (doubles): 16-byte aligned pairs, rows on different banks
constexpr int FJ = 16, TR = 128;                   // column sums: features per workgroup, rows per tile

struct alignas(16) Row { int state, x, y, id; };   // state: 0 none, 1 statistics only, 2 live
enum { H_NSTAT = 0, H_NLIVE = 1, H_SKIPPED = 2, H_DEGENERATE = 3, H_M = 4, H_INTS = 8 };

struct Sections { size_t hdr, rows, stat, live, stats, E, Hh, Z, lse, ce, hit, dZ, dE, total; };
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline Sections sections(long R, int D, bool grad) {
    Sections s;
    s.hdr = 0;
    s.rows = up16(H_INTS * sizeof(int));
    s.stat = s.rows + (size_t)R * sizeof(Row);
    s.live = up16(s.stat + (size_t)R * sizeof(int));
    s.stats = up16(s.live + (size_t)R * sizeof(int));
    s.E = s.stats + (size_t)4 * D * sizeof(double);          // mean, sd, sum dxhat, sum dxhat xhat
    s.Hh = s.E + (size_t)R * D * sizeof(double);
    s.Z = s.Hh + (size_t)R * D * sizeof(double);
    s.lse = s.Z + (size_t)R * D * sizeof(double);
    s.ce = s.lse + (size_t)R * sizeof(double);
    s.hit = s.ce + (size_t)R * sizeof(double);
    s.dZ = up16(s.hit + (size_t)R * sizeof(int));
    s.dE = s.dZ + (grad ? (size_t)R * D * sizeof(double) : 0);
    s.total = s.dE + (grad ? (size_t)R * D * sizeof(double) : 0);
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(THREADS) void row_kernel(const double* __restrict__ boxes, const long long* __restrict__ ids, const int* __restrict__ count,
                                                      long R, int Gmax, int H, int W, int K, double stride, int round_centre, int padded,
                                                      long long ignore_index, Row* __restrict__ rows, double* __restrict__ per_row) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= R) return;
    const int n = (int)(i / Gmax), g = (int)(i - (long)n * Gmax);
    Row r;
    r.state = 0; r.x = 0; r.y = 0; r.id = -1;
    if (g >= min(max(count[n], 0), Gmax)) {
        if (padded) r.state = 1;                              // the reference's zero box: cell (0, 0) of its image, in the statistics only
    } else {
        const long long id = ids[i];
        if (id != ignore_index) {
            const double* const b = boxes + i * 4;
            const double cx = (b[0] + b[2] / 2.0) / stride, cy = (b[1] + b[3] / 2.0) / stride;
            const double x = round_centre ? rint(cx) : trunc(cx), y = round_centre ? rint(cy) : trunc(cy);
            // (every comparison is false for a NaN: a non-finite number anywhere skips the row)
            const bool finite = fabs(b[0]) < __builtin_inf() && fabs(b[1]) < __builtin_inf() && b[2] < __builtin_inf() && b[3] < __builtin_inf();
            if (finite && b[2] >= 0.0 && b[3] >= 0.0 && x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1) && id >= 0 && id < K) {
                r.state = 2; r.x = (int)x; r.y = (int)y; r.id = (int)id;
            } else {
                r.state = -1;                                 // skipped: counted, then cleared by count_kernel
            }
        }
    }
    rows[i] = r;
    if (per_row && r.state != 2) per_row[i] = 0.0;
}

// the stat rows and the live rows, compacted in row order; counts.  One workgroup.
__global__ __launch_bounds__(THREADS) void count_kernel(Row* __restrict__ rows, long R, int training, int* __restrict__ stat, int* __restrict__ live,
                                                        int* __restrict__ hdr, double* __restrict__ per_row, int* __restrict__ skipped) {
    __shared__ int s_cnt[3][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n_stat = 0, n_live = 0, n_skip = 0;
    for (long base = 0; base < R; base += THREADS) {
        const long i = base + tid;
        int st = 0;
        if (i < R) st = rows[i].state;
        const unsigned long long v_stat = __ballot(st >= 1), v_live = __ballot(st == 2), v_skip = __ballot(st < 0);
        __syncthreads();
        if (lane == 0) { s_cnt[0][wave] = __popcll(v_stat); s_cnt[1][wave] = __popcll(v_live); s_cnt[2][wave] = __popcll(v_skip); }
        __syncthreads();
        int b_stat = 0, b_live = 0, t_stat = 0, t_live = 0, t_skip = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) { b_stat += s_cnt[0][w]; b_live += s_cnt[1][w]; }
            t_stat += s_cnt[0][w]; t_live += s_cnt[1][w]; t_skip += s_cnt[2][w];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (st >= 1) stat[n_stat + b_stat + __popcll(v_stat & below)] = (int)i;
        if (st == 2) live[n_live + b_live + __popcll(v_live & below)] = (int)i;
        if (st < 0) rows[i].state = 0;
        n_stat += t_stat; n_live += t_live; n_skip += t_skip;
    }
    const int degenerate = training && n_stat < 2;
    if (degenerate) {                                         // nothing to normalise over: value 0, gradients 0, running statistics kept
        for (long i = tid; i < R; i += THREADS)
            if (rows[i].state > 0) {
                if (rows[i].state == 2 && per_row) per_row[i] = 0.0;
                rows[i].state = 0;
            }
    }
    if (tid == 0) {
        hdr[H_NSTAT] = degenerate ? 0 : n_stat; hdr[H_NLIVE] = degenerate ? 0 : n_live; hdr[H_SKIPPED] = n_skip; hdr[H_DEGENERATE] = degenerate;
        hdr[H_M] = n_live;
        if (skipped) skipped[0] = n_skip;
    }
}

__global__ __launch_bounds__(THREADS) void gather_kernel(const float* __restrict__ reid, long sn, long sc, long sh, long sw, const Row* __restrict__ rows,
                                                         long R, int Gmax, int D, double* __restrict__ E) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= R * D) return;
    const long r = e / D;
    const int i = (int)(e - r * D);
    const Row row = rows[r];
    if (row.state < 1) return;
    E[e] = (double)reid[(r / Gmax) * sn + (long)i * sc + (long)row.y * sh + (long)row.x * sw];
}

__global__ __launch_bounds__(THREADS) void hidden_kernel(const double* __restrict__ E, const float* __restrict__ W1, const Row* __restrict__ rows, long R,
                                                         int D, double* __restrict__ Hh) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= R * D) return;
    const long r = e / D;
    const int j = (int)(e - r * D);
    if (rows[r].state < 1) return;
    const double* const x = E + r * D;
    const float* const w = W1 + (long)j * D;
    double acc = 0.0;
    for (int i = 0; i < D; ++i) acc = fma((double)w[i], x[i], acc);
    Hh[e] = acc;
}

// sum over the rows of `list` (n entries, in list order) of val(row, j) for the workgroup's FJ features: TR-row tiles through LDS, then one thread per
// feature adds the tile's values in order.  Valid in threads 0 .. FJ-1 (feature j0 + tid).
template <class F>
__device__ __forceinline__ double column_sum(const int* __restrict__ list, int n, int j0, int D, double* s_t, F val) {
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int base = 0; base < n; base += TR) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TR * FJ / THREADS; ++u) {
            const int e = u * THREADS + tid, rl = e / FJ, jj = e % FJ;
            double v = 0.0;
            if (base + rl < n && j0 + jj < D) v = val((long)list[base + rl], j0 + jj);
            s_t[rl * (FJ + 1) + jj] = v;
        }
        __syncthreads();
        if (tid < FJ) {
            const int m = min(TR, n - base);
            for (int rl = 0; rl < m; ++rl) sum += s_t[rl * (FJ + 1) + tid];
        }
    }
    return sum;
}

__global__ __launch_bounds__(THREADS) void bn_stats_kernel(const double* __restrict__ Hh, const int* __restrict__ stat, const int* __restrict__ hdr, int D,
                                                           int training, double bn_eps, double momentum, const float* __restrict__ running_mean,
                                                           const float* __restrict__ running_var, double* __restrict__ stats,
                                                           float* __restrict__ new_stats) {
    __shared__ double s_t[TR * (FJ + 1)];
    __shared__ double s_mean[FJ];
    const int tid = threadIdx.x, j0 = blockIdx.x * FJ, j = j0 + tid;
    const bool mine = tid < FJ && j < D;
    const int n = hdr[H_NSTAT];
    if (!training || n < 2) {                                 // the running statistics, unchanged
        if (mine) {
            stats[j] = (double)running_mean[j];
            stats[D + j] = sqrt((double)running_var[j] + bn_eps);
            if (new_stats) { new_stats[j] = running_mean[j]; new_stats[D + j] = running_var[j]; }
        }
        return;
    }
    const double total = column_sum(stat, n, j0, D, s_t, [&](long r, int jj) { return Hh[r * D + jj]; });
    const double mean = total / (double)n;
    if (tid < FJ) s_mean[tid] = mean;
    __syncthreads();
    const double sq = column_sum(stat, n, j0, D, s_t, [&](long r, int jj) { const double d = Hh[r * D + jj] - s_mean[jj - j0]; return d * d; });
    if (mine) {
        const double var = sq / (double)n;
        stats[j] = mean;
        stats[D + j] = sqrt(var + bn_eps);
        if (new_stats) {
            new_stats[j] = (float)((1.0 - momentum) * (double)running_mean[j] + momentum * mean);
            new_stats[D + j] = (float)((1.0 - momentum) * (double)running_var[j] + momentum * (var * (double)n / (double)(n - 1)));
        }
    }
}

__global__ __launch_bounds__(THREADS) void act_kernel(const double* __restrict__ Hh, const Row* __restrict__ rows, const double* __restrict__ stats,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, long R, int D,
                                                      double* __restrict__ Z) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= R * D) return;
    const long r = e / D;
    const int j = (int)(e - r * D);
    if (rows[r].state != 2) return;
    const double a = (Hh[e] - stats[j]) / stats[D + j] * (double)gamma[j] + (double)beta[j];
    Z[e] = fmax(a, 0.0);
}

// ---------------------------------------------------------------------------------------------------------------- logits
// The logits of the block's RB rows (s_row: row index or -1) against identities k0 .. k0 + KT - 1: thread (rq = tid / 16, kq = tid % 16) holds rows
// 2 rq, 2 rq + 1 x identities k0 + 4 kq .. + 3.  logit = b2[k], then fma(z_j, W2[k, j], logit) for j ascending; -inf beyond K.
__device__ __forceinline__ void logits_tile(const double* __restrict__ Z, const int* s_row, const float* __restrict__ W2, const float* __restrict__ b2,
                                            int D, int K, int k0, double* s_z, double* s_w, double (&acc)[2][4]) {
    const int tid = threadIdx.x, kq = tid & 15, rq = tid >> 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = k0 + kq * 4 + c;
        acc[0][c] = acc[1][c] = k < K ? (double)b2[k] : -__builtin_inf();
    }
    for (int j0 = 0; j0 < D; j0 += DC) {
        __syncthreads();                                      // the readers of the previous chunk are done
#pragma unroll
        for (int u = 0; u < RB * DC / THREADS; ++u) {
            const int e = u * THREADS + tid, jj = e % DC, rl = e / DC;
            const int r = s_row[rl];
            s_z[jj * ZS_LD + rl] = (r >= 0 && j0 + jj < D) ? Z[(long)r * D + j0 + jj] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < KT * DC / THREADS; ++u) {
            const int e = u * THREADS + tid, jj = e % DC, kk = e / DC;
            const int k = k0 + kk;
            s_w[jj * WS_LD + kk] = (k < K && j0 + jj < D) ? (double)W2[(long)k * D + j0 + jj] : 0.0;
        }
        __syncthreads();
        const int jn = min(DC, D - j0);
#pragma unroll 2
        for (int jj = 0; jj < jn; ++jj) {
            const double2 z = *reinterpret_cast<const double2*>(s_z + jj * ZS_LD + rq * 2);
            const double2 wa = *reinterpret_cast<const double2*>(s_w + jj * WS_LD + kq * 4);
            const double2 wb = *reinterpret_cast<const double2*>(s_w + jj * WS_LD + kq * 4 + 2);
            const double w[4] = {wa.x, wa.y, wb.x, wb.y};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[0][c] = fma(z.x, w[c], acc[0][c]);
                acc[1][c] = fma(z.y, w[c], acc[1][c]);
            }
        }
    }
}

__device__ __forceinline__ void block_rows(const int* __restrict__ live, const Row* __restrict__ rows, int base, int n_live, int* s_row, int* s_id) {
    const int tid = threadIdx.x;
    if (tid < RB) {
        const int r = base + tid < n_live ? live[base + tid] : -1;
        s_row[tid] = r;
        s_id[tid] = r >= 0 ? rows[r].id : -1;
    }
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void ce_kernel(const double* __restrict__ Z, const int* __restrict__ live, const Row* __restrict__ rows,
                                                     const int* __restrict__ hdr, const float* __restrict__ W2, const float* __restrict__ b2, int D, int K,
                                                     double* __restrict__ lse, double* __restrict__ ce, int* __restrict__ hit,
                                                     double* __restrict__ per_row) {
    __shared__ __attribute__((aligned(16))) double s_z[DC * ZS_LD];
    __shared__ __attribute__((aligned(16))) double s_w[DC * WS_LD];
    __shared__ int s_row[RB], s_id[RB];
    const int n_live = hdr[H_NLIVE], base = blockIdx.x * RB;
    if (base >= n_live) return;                               // (uniform)
    block_rows(live, rows, base, n_live, s_row, s_id);
    const int tid = threadIdx.x, kq = tid & 15, rq = tid >> 4;
    double run_m[2] = {-__builtin_inf(), -__builtin_inf()}, run_s[2] = {0.0, 0.0}, best[2] = {-__builtin_inf(), -__builtin_inf()}, lid[2] = {0.0, 0.0};
    int best_k[2] = {0, 0};
    for (int k0 = 0; k0 < K; k0 += KT) {                      // tiles in ascending order
        double acc[2][4];
        logits_tile(Z, s_row, W2, b2, D, K, k0, s_z, s_w, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double tm = acc[i][0];
            int tk = k0 + kq * 4;
#pragma unroll
            for (int c = 1; c < 4; ++c)
                if (acc[i][c] > tm) { tm = acc[i][c]; tk = k0 + kq * 4 + c; }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {          // the 16 lanes of a row: the larger value, the smaller index on a tie
                const double om = __shfl_xor(tm, off);
                const int ok = __shfl_xor(tk, off);
                if (om > tm || (om == tm && ok < tk)) { tm = om; tk = ok; }
            }
            if (tm > best[i]) { best[i] = tm; best_k[i] = tk; }      // the first of the largest
            const double m = fmax(run_m[i], tm);
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) s += exp(acc[i][c] - m);
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off);
            run_s[i] = run_s[i] * exp(run_m[i] - m) + s;
            run_m[i] = m;
            const int c_id = s_id[rq * 2 + i] - (k0 + kq * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c == c_id) lid[i] = acc[i][c];
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        double v = lid[i];                                    // one lane holds it, the others 0
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
        const int r = s_row[rq * 2 + i];
        if (kq == 0 && r >= 0) {
            const double l = run_m[i] + log(run_s[i]);
            lse[r] = l;
            ce[r] = l - v;
            hit[r] = best_k[i] == s_id[rq * 2 + i];
            if (per_row) per_row[r] = l - v;
        }
    }
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const double* __restrict__ ce, const int* __restrict__ hit, const int* __restrict__ live,
                                                         const int* __restrict__ hdr, int training, double* __restrict__ total, int* __restrict__ counts) {
    __shared__ double s_v[THREADS];
    __shared__ int s_h[THREADS];
    const int tid = threadIdx.x, n = hdr[H_NLIVE];
    double sum = 0.0;
    int correct = 0;
    for (int base = 0; base < n; base += THREADS) {
        __syncthreads();
        const int r = base + tid < n ? live[base + tid] : -1;
        s_v[tid] = r >= 0 ? ce[r] : 0.0;
        s_h[tid] = r >= 0 ? hit[r] : 0;
        __syncthreads();
        if (tid == 0) {
            const int m = min(THREADS, n - base);
            for (int i = 0; i < m; ++i) { sum += s_v[i]; correct += s_h[i]; }
        }
    }
    if (tid == 0) {
        if (total) total[0] = sum / ((double)hdr[H_M] + 1e-8);
        if (counts) {
            counts[0] = hdr[H_M]; counts[1] = correct; counts[2] = hdr[H_SKIPPED];
            counts[3] = training && !hdr[H_DEGENERATE];      // the running statistics made a step
        }
    }
}

// ================================================================================================================ gradient
// g[r, k] = scale (exp(logit - lse_r) - [k == id_r]) / (M + 1e-8) of the thread's 2 x 4 logits -> s_g[r][k] (pitch KT + 2)
__device__ __forceinline__ void store_g(const double (&acc)[2][4], const int* s_row, const int* s_id, const double* __restrict__ lse, double factor, int k0,
                                        double* s_g) {
    const int tid = threadIdx.x, kq = tid & 15, rq = tid >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int rl = rq * 2 + i, r = s_row[rl];
        const double l = r >= 0 ? lse[r] : 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = k0 + kq * 4 + c;
            double g = 0.0;
            if (r >= 0) g = factor * (exp(acc[i][c] - l) - (k == s_id[rl] ? 1.0 : 0.0));      // (-inf beyond K: exp gives 0)
            s_g[rl * WS_LD + kq * 4 + c] = g;
        }
    }
}

template <int CHUNKS>      // CHUNKS * DC >= D
__global__ __launch_bounds__(THREADS) void dz_kernel(const double* __restrict__ Z, const int* __restrict__ live, const Row* __restrict__ rows,
                                                     const int* __restrict__ hdr, const float* __restrict__ W2, const float* __restrict__ b2, int D, int K,
                                                     const double* __restrict__ lse, const double* __restrict__ scale, double* __restrict__ dZ) {
    __shared__ __attribute__((aligned(16))) double s_z[DC * ZS_LD];
    constexpr int W3_LD = DC + 2;
    static_assert(KT * W3_LD >= DC * WS_LD, "both forms of the chunk fit the buffer");
    __shared__ __attribute__((aligned(16))) double s_w[KT * W3_LD];      // phase 1: [feature][identity]; phase 3: [identity][feature], pitch DC + 2
    __shared__ __attribute__((aligned(16))) double s_g[RB * WS_LD];
    __shared__ int s_row[RB], s_id[RB];
    const int n_live = hdr[H_NLIVE], base = blockIdx.x * RB;
    if (base >= n_live) return;
    block_rows(live, rows, base, n_live, s_row, s_id);
    const int tid = threadIdx.x;
    const int rr = tid >> 3, jq = tid & 7;                    // phase 3: row rr, features 4 jq .. 4 jq + 3 of each chunk
    const double factor = (scale ? scale[0] : 1.0) / ((double)hdr[H_M] + 1e-8);
    double out[CHUNKS][4];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[c][q] = 0.0;
    for (int k0 = 0; k0 < K; k0 += KT) {
        double acc[2][4];
        logits_tile(Z, s_row, W2, b2, D, K, k0, s_z, s_w, acc);
        store_g(acc, s_row, s_id, lse, factor, k0, s_g);
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int j0 = c * DC;
            if (j0 >= D) break;
            __syncthreads();                                  // s_g written, the previous readers of s_w done
#pragma unroll
            for (int u = 0; u < KT * DC / THREADS; ++u) {
                const int e = u * THREADS + tid, jj = e % DC, kk = e / DC;
                const int k = k0 + kk;
                s_w[kk * W3_LD + jj] = (k < K && j0 + jj < D) ? (double)W2[(long)k * D + j0 + jj] : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int kk = 0; kk < KT; ++kk) {                 // k ascending
                const double g = s_g[rr * WS_LD + kk];
                const double2 wa = *reinterpret_cast<const double2*>(s_w + kk * W3_LD + jq * 4);
                const double2 wb = *reinterpret_cast<const double2*>(s_w + kk * W3_LD + jq * 4 + 2);
                out[c][0] = fma(g, wa.x, out[c][0]); out[c][1] = fma(g, wa.y, out[c][1]);
                out[c][2] = fma(g, wb.x, out[c][2]); out[c][3] = fma(g, wb.y, out[c][3]);
            }
        }
    }
    const int r = s_row[rr];
    if (r >= 0) {
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = c * DC + jq * 4 + q;
                if (j < D) dZ[(long)r * D + j] = out[c][q];
            }
    }
}

template <int CHUNKS>
__global__ __launch_bounds__(THREADS) void dw2_kernel(const double* __restrict__ Z, const int* __restrict__ live, const Row* __restrict__ rows,
                                                      const int* __restrict__ hdr, const float* __restrict__ W2, const float* __restrict__ b2, int D, int K,
                                                      const double* __restrict__ lse, const double* __restrict__ scale, float* __restrict__ dW2,
                                                      float* __restrict__ db2) {
    __shared__ __attribute__((aligned(16))) double s_z[DC * ZS_LD];      // phase 1: [feature][row]; phase 3: [row][feature], pitch DC + 2
    __shared__ __attribute__((aligned(16))) double s_w[DC * WS_LD];
    __shared__ __attribute__((aligned(16))) double s_g[RB * WS_LD];
    __shared__ int s_row[RB], s_id[RB];
    constexpr int Z3_LD = DC + 2;
    static_assert(RB * Z3_LD <= DC * ZS_LD, "the transposed chunk fits the same buffer");
    const int n_live = hdr[H_NLIVE], k0 = blockIdx.x * KT;
    const int tid = threadIdx.x;
    const int kk = tid >> 2, jq = tid & 3;                    // phase 3: identity k0 + kk, features 8 jq .. 8 jq + 7 of each chunk
    const double factor = (scale ? scale[0] : 1.0) / ((double)hdr[H_M] + 1e-8);
    double out[CHUNKS][8], bias = 0.0;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
        for (int q = 0; q < 8; ++q) out[c][q] = 0.0;
    for (int base = 0; base < n_live; base += RB) {           // all live rows, in order
        __syncthreads();                                      // the readers of s_row / s_g of the previous block of rows are done
        block_rows(live, rows, base, n_live, s_row, s_id);
        double acc[2][4];
        logits_tile(Z, s_row, W2, b2, D, K, k0, s_z, s_w, acc);
        store_g(acc, s_row, s_id, lse, factor, k0, s_g);
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int j0 = c * DC;
            if (j0 >= D) break;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < RB * DC / THREADS; ++u) {
                const int e = u * THREADS + tid, jj = e % DC, rl = e / DC;
                const int r = s_row[rl];
                s_z[rl * Z3_LD + jj] = (r >= 0 && j0 + jj < D) ? Z[(long)r * D + j0 + jj] : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int rl = 0; rl < RB; ++rl) {                 // r ascending
                const double g = s_g[rl * WS_LD + kk];
                if (c == 0 && jq == 0) bias += g;
                const double* const zr = s_z + rl * Z3_LD + jq * 8;
#pragma unroll
                for (int q = 0; q < 8; q += 2) {
                    const double2 z = *reinterpret_cast<const double2*>(zr + q);
                    out[c][q] = fma(g, z.x, out[c][q]);
                    out[c][q + 1] = fma(g, z.y, out[c][q + 1]);
                }
            }
        }
    }
    const int k = k0 + kk;
    if (k < K) {
        if (dW2) {
#pragma unroll
            for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int j = c * DC + jq * 8 + q;
                    if (j < D) dW2[(long)k * D + j] = (float)out[c][q];
                }
        }
        if (db2 && jq == 0) db2[k] = (float)bias;
    }
}

// dbeta, dgamma, and the sums the BatchNorm backward needs: over the live rows in order (dZ is 0 on every other row)
__global__ __launch_bounds__(THREADS) void bn_grad_kernel(const double* __restrict__ Hh, const double* __restrict__ Z, const double* __restrict__ dZ,
                                                          const int* __restrict__ live, const int* __restrict__ hdr, int D, const float* __restrict__ gamma,
                                                          double* __restrict__ stats, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double s_t[TR * (FJ + 1)];
    const int tid = threadIdx.x, j0 = blockIdx.x * FJ, j = j0 + tid;
    const int n = hdr[H_NLIVE];
    const double s_da = column_sum(live, n, j0, D, s_t, [&](long r, int jj) { return Z[r * D + jj] > 0.0 ? dZ[r * D + jj] : 0.0; });
    const double s_dax = column_sum(live, n, j0, D, s_t, [&](long r, int jj) {
        return Z[r * D + jj] > 0.0 ? dZ[r * D + jj] * ((Hh[r * D + jj] - stats[jj]) / stats[D + jj]) : 0.0;
    });
    if (tid < FJ && j < D) {
        if (dbeta) dbeta[j] = (float)s_da;
        if (dgamma) dgamma[j] = (float)s_dax;
        stats[2 * D + j] = s_da * (double)gamma[j];           // sum dxhat
        stats[3 * D + j] = s_dax * (double)gamma[j];          // sum dxhat xhat
    }
}

// dH of every stat row, written over dZ's row (a stat row that is not live has dZ = 0 but, in training, a dH through the batch statistics)
__global__ __launch_bounds__(THREADS) void dh_kernel(const double* __restrict__ Hh, const double* __restrict__ Z, const Row* __restrict__ rows,
                                                     const double* __restrict__ stats, const float* __restrict__ gamma, const int* __restrict__ hdr, long R,
                                                     int D, int training, double* __restrict__ dZ) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= R * D) return;
    const long r = e / D;
    const int j = (int)(e - r * D);
    const int st = rows[r].state;
    if (st < 1) return;
    const double sd = stats[D + j];
    const double dxhat = (st == 2 && Z[e] > 0.0) ? dZ[e] * (double)gamma[j] : 0.0;
    double dh;
    if (training) {
        const double n = (double)hdr[H_NSTAT];
        const double xhat = (Hh[e] - stats[j]) / sd;
        dh = (n * dxhat - stats[2 * D + j] - xhat * stats[3 * D + j]) / (n * sd);
    } else {
        dh = dxhat / sd;
    }
    dZ[e] = dh;
}

// dW1[j, i] = sum over the stat rows in order of dH[r, j] E[r, i]: a workgroup per 16 x 16 tile, 64-row tiles through LDS
__global__ __launch_bounds__(THREADS) void dw1_kernel(const double* __restrict__ dH, const double* __restrict__ E, const int* __restrict__ stat,
                                                      const int* __restrict__ hdr, int D, float* __restrict__ dW1) {
    constexpr int T = 16, ROWS = 64;
    __shared__ double s_h[ROWS * (T + 1)], s_e[ROWS * (T + 1)];
    const int tid = threadIdx.x, tj = tid / T, ti = tid % T;
    const int tiles = (D + T - 1) / T;
    const int j0 = (blockIdx.x / tiles) * T, i0 = (blockIdx.x % tiles) * T;
    const int n = hdr[H_NSTAT];
    double acc = 0.0;
    for (int base = 0; base < n; base += ROWS) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < ROWS * T / THREADS; ++u) {
            const int e = u * THREADS + tid, rl = e / T, c = e % T;
            const bool ok = base + rl < n;
            const long r = ok ? stat[base + rl] : 0;
            s_h[rl * (T + 1) + c] = (ok && j0 + c < D) ? dH[r * D + j0 + c] : 0.0;
            s_e[rl * (T + 1) + c] = (ok && i0 + c < D) ? E[r * D + i0 + c] : 0.0;
        }
        __syncthreads();
        const int m = min(ROWS, n - base);
        for (int rl = 0; rl < m; ++rl) acc = fma(s_h[rl * (T + 1) + tj], s_e[rl * (T + 1) + ti], acc);
    }
    if (j0 + tj < D && i0 + ti < D) dW1[(long)(j0 + tj) * D + i0 + ti] = (float)acc;
}

__global__ __launch_bounds__(THREADS) void de_kernel(const double* __restrict__ dH, const float* __restrict__ W1, const Row* __restrict__ rows, long R,
                                                     int D, double* __restrict__ dE) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= R * D) return;
    const long r = e / D;
    const int i = (int)(e - r * D);
    if (rows[r].state < 1) return;
    const double* const g = dH + r * D;
    double acc = 0.0;
    for (int j = 0; j < D; ++j) acc = fma((double)W1[(long)j * D + i], g[j], acc);
    dE[e] = acc;
}

struct ScatterArgs {
    float* grad; long gn, gc, gh, gw;
    const Row* rows;
    const double* dE;
    int D, H, W, Gmax, tx;
    int cminor;                                    // the gradient's channel stride is 1: lanes along the channels of a pixel
};

__global__ __launch_bounds__(THREADS) void scatter_kernel(const ScatterArgs a) {
    __shared__ int4 s_hit[PASS_SLOTS];             // x, y, slot
    __shared__ int s_cnt[WAVES];
    const Tile tile(blockIdx.x, a.tx, a.H, a.W);
    const Row* const rows = a.rows + (long)tile.n * a.Gmax;
    const double* const dE = a.dE + (long)tile.n * a.Gmax * a.D;
    float* const grad = a.grad + (long)tile.n * a.gn;
    const int passes = (a.Gmax + PASS_SLOTS - 1) / PASS_SLOTS;
    int cnt = 0;
    // THREADS * D elements, THREADS per step: the trip count is D in every thread, so the barriers are uniform
    for (int step = 0; step < a.D; ++step) {
        const Elem e = element(a.cminor, tile, step, a.D);
        const bool inside = tile.holds(e.x, e.y);
        double sum = 0.0;
        bool touched = false;
        for (int p = 0; p < passes; ++p) {
            if (passes > 1 || step == 0) {                    // a single pass is staged once and stays
                cnt = stage_pass(p * PASS_SLOTS, a.Gmax, s_hit, s_cnt, [&](int s, int4& v) {
                    const Row r = rows[s];
                    v = make_int4(r.x, r.y, s, 0);
                    return r.state >= 1 && r.x >= tile.x0 && r.x < tile.x1 && r.y >= tile.y0 && r.y < tile.y1;
                });
            }
            if (inside) {
                for (int q = 0; q < cnt; ++q) {               // slot order
                    const int4 h = s_hit[q];
                    if (h.x == e.x && h.y == e.y) { sum += dE[(long)h.z * a.D + e.c]; touched = true; }
                }
            }
        }
        if (inside) grad[(long)e.c * a.gc + (long)e.y * a.gh + (long)e.x * a.gw] = touched ? (float)sum : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct Call {
    const float* reid; int64_t sn, sc, sh, sw;
    int N, D, H, W, Gmax, K;
    const double* boxes; const int64_t* ids; const int32_t* count;
    const float *W1, *gamma, *beta, *running_mean, *running_var, *W2, *b2;
    const cnl_reid_loss_params* p;
};

inline int check_call(const Call& c, const char* who) {
    CNL_REQUIRE(c.p, CNL_E_BAD_ARG, "%s: null params", who);
    if (int rc = check_dims(who, c.N, c.H, c.W, c.Gmax)) return rc;
    CNL_REQUIRE(c.D >= 1 && c.D <= MAX_D, CNL_E_BAD_ARG, "%s: D = %d outside 1..%d", who, c.D, MAX_D);
    CNL_REQUIRE(c.K >= 2 && c.K <= MAX_K, CNL_E_BAD_ARG, "%s: K = %d outside 2..2^20", who, c.K);
    if (int rc = check_stride(who, c.p->stride)) return rc;
    CNL_REQUIRE(c.p->bn_eps > 0.0 && c.p->bn_eps < 1e6, CNL_E_BAD_ARG, "%s: bn_eps = %g must be positive", who, c.p->bn_eps);
    CNL_REQUIRE(c.p->momentum >= 0.0 && c.p->momentum <= 1.0, CNL_E_BAD_ARG, "%s: momentum = %g outside 0..1", who, c.p->momentum);
    CNL_REQUIRE((c.p->center == 0 || c.p->center == 1) && (c.p->padded_rows == 0 || c.p->padded_rows == 1) && (c.p->training == 0 || c.p->training == 1),
                CNL_E_BAD_ARG, "%s: center, padded_rows and training are 0 or 1", who);
    if (c.N == 0) return CNL_OK;
    CNL_REQUIRE(c.reid && c.boxes && c.ids && c.count && c.W1 && c.gamma && c.beta && c.running_mean && c.running_var && c.W2 && c.b2, CNL_E_BAD_ARG,
                "%s: null pointer", who);
    return check_aligned(who, {c.boxes, c.ids}, nullptr, {c.reid, c.count, c.W1, c.gamma, c.beta, c.running_mean, c.running_var, c.W2, c.b2});
}

inline unsigned blocks_for(long n) { return (unsigned)((n + THREADS - 1) / THREADS); }

// rows, lists, E, H, statistics, Z, and ce_kernel: everything the value and the gradient share
inline int forward(const Call& c, char* ws, const Sections& sec, double* per_row, float* new_stats, int* skipped, hipStream_t st) {
    const long R = (long)c.N * c.Gmax;
    const int D = c.D;
    int* const hdr = reinterpret_cast<int*>(ws + sec.hdr);
    Row* const rows = reinterpret_cast<Row*>(ws + sec.rows);
    int* const stat = reinterpret_cast<int*>(ws + sec.stat);
    int* const live = reinterpret_cast<int*>(ws + sec.live);
    double* const stats = reinterpret_cast<double*>(ws + sec.stats);
    double* const E = reinterpret_cast<double*>(ws + sec.E);
    double* const Hh = reinterpret_cast<double*>(ws + sec.Hh);
    double* const Z = reinterpret_cast<double*>(ws + sec.Z);
    double* const lse = reinterpret_cast<double*>(ws + sec.lse);
    double* const ce = reinterpret_cast<double*>(ws + sec.ce);
    int* const hit = reinterpret_cast<int*>(ws + sec.hit);
    const cnl_reid_loss_params* const p = c.p;

    hipLaunchKernelGGL(row_kernel, dim3(blocks_for(R)), dim3(THREADS), 0, st, c.boxes, reinterpret_cast<const long long*>(c.ids), c.count, R, c.Gmax, c.H,
                       c.W, c.K, p->stride, p->center, p->padded_rows, (long long)p->ignore_index, rows, per_row);
    if (int rc = cnl::check_launch("reid_loss row_kernel")) return rc;
    hipLaunchKernelGGL(count_kernel, dim3(1), dim3(THREADS), 0, st, rows, R, p->training, stat, live, hdr, per_row, skipped);
    if (int rc = cnl::check_launch("reid_loss count_kernel")) return rc;
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(R * D)), dim3(THREADS), 0, st, c.reid, (long)c.sn, (long)c.sc, (long)c.sh, (long)c.sw, rows, R, c.Gmax,
                       D, E);
    if (int rc = cnl::check_launch("reid_loss gather_kernel")) return rc;
    hipLaunchKernelGGL(hidden_kernel, dim3(blocks_for(R * D)), dim3(THREADS), 0, st, E, c.W1, rows, R, D, Hh);
    if (int rc = cnl::check_launch("reid_loss hidden_kernel")) return rc;
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)((D + FJ - 1) / FJ)), dim3(THREADS), 0, st, Hh, stat, hdr, D, p->training, p->bn_eps, p->momentum,
                       c.running_mean, c.running_var, stats, new_stats);
    if (int rc = cnl::check_launch("reid_loss bn_stats_kernel")) return rc;
    hipLaunchKernelGGL(act_kernel, dim3(blocks_for(R * D)), dim3(THREADS), 0, st, Hh, rows, stats, c.gamma, c.beta, R, D, Z);
    if (int rc = cnl::check_launch("reid_loss act_kernel")) return rc;
    hipLaunchKernelGGL(ce_kernel, dim3((unsigned)((R + RB - 1) / RB)), dim3(THREADS), 0, st, Z, live, rows, hdr, c.W2, c.b2, D, c.K, lse, ce, hit, per_row);
    return cnl::check_launch("reid_loss ce_kernel");
}

}  // namespace cnl_reid_loss

static size_t reid_ws_bytes(int32_t N, int32_t Gmax, int32_t D, bool grad) {
    using namespace cnl_reid_loss;
    return slots_in_range(N, Gmax) && D >= 1 && D <= MAX_D ? sections((long)N * Gmax, D, grad).total : 0;
}

extern "C" size_t cnl_reid_loss_workspace_bytes(int32_t N, int32_t Gmax, int32_t D) { return reid_ws_bytes(N, Gmax, D, false); }
extern "C" size_t cnl_reid_loss_grad_workspace_bytes(int32_t N, int32_t Gmax, int32_t D) { return reid_ws_bytes(N, Gmax, D, true); }

extern "C" int cnl_reid_loss_f64(const float* reid, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int32_t N, int32_t D, int32_t H, int32_t W,
                                 const double* gt_boxes, const int64_t* gt_ids, const int32_t* gt_count, int32_t Gmax, const float* W1, const float* gamma,
                                 const float* beta, const float* running_mean, const float* running_var, const float* W2, const float* b2, int32_t K,
                                 const cnl_reid_loss_params* p, double* per_row, double* total, int32_t* counts, float* new_stats, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    using namespace cnl_reid_loss;
    const char* const who = "cnl_reid_loss_f64";
    const Call c{reid, sn, sc, sh, sw, N, D, H, W, Gmax, K, gt_boxes, gt_ids, gt_count, W1, gamma, beta, running_mean, running_var, W2, b2, p};
    if (int rc = check_call(c, who)) return rc;
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(per_row && total && counts && workspace, CNL_E_BAD_ARG, "%s: null pointer", who);
    if (int rc = check_aligned(who, {per_row, total}, workspace, {counts, new_stats})) return rc;
    const long R = (long)N * Gmax;
    CNL_REQUIRE(R < (1l << 31) / MAX_D, CNL_E_UNSUPPORTED, "%s: %ld rows exceed the grid", who, R);
    const Sections sec = sections(R, D, false);
    if (int rc = check_workspace(who, workspace_bytes, sec.total)) return rc;
    char* const ws = static_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = forward(c, ws, sec, per_row, new_stats, nullptr, st)) return rc;
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(THREADS), 0, st, reinterpret_cast<const double*>(ws + sec.ce), reinterpret_cast<const int*>(ws + sec.hit),
                       reinterpret_cast<const int*>(ws + sec.live), reinterpret_cast<const int*>(ws + sec.hdr), p->training, total, counts);
    return cnl::check_launch("reid_loss finish_kernel");
}

extern "C" int cnl_reid_loss_grad_f32(const float* reid, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int32_t N, int32_t D, int32_t H, int32_t W,
                                      const double* gt_boxes, const int64_t* gt_ids, const int32_t* gt_count, int32_t Gmax, const float* W1,
                                      const float* gamma, const float* beta, const float* running_mean, const float* running_var, const float* W2,
                                      const float* b2, int32_t K, const cnl_reid_loss_params* p, const double* scale, float* grad_reid, int64_t gn,
                                      int64_t gc, int64_t gh, int64_t gw, float* grad_W1, float* grad_gamma, float* grad_beta, float* grad_W2,
                                      float* grad_b2, int32_t* skipped, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace cnl_reid_loss;
    const char* const who = "cnl_reid_loss_grad_f32";
    const Call c{reid, sn, sc, sh, sw, N, D, H, W, Gmax, K, gt_boxes, gt_ids, gt_count, W1, gamma, beta, running_mean, running_var, W2, b2, p};
    if (int rc = check_call(c, who)) return rc;
    if (N == 0) return CNL_OK;      // (the parameter gradients of an empty batch are the caller's zeros)
    CNL_REQUIRE(workspace, CNL_E_BAD_ARG, "%s: null pointer", who);
    if (int rc = check_aligned(who, {scale}, workspace, {grad_reid, grad_W1, grad_gamma, grad_beta, grad_W2, grad_b2, skipped})) return rc;
    const long R = (long)N * Gmax;
    CNL_REQUIRE(R < (1l << 31) / MAX_D, CNL_E_UNSUPPORTED, "%s: %ld rows exceed the grid", who, R);
    int tiles;
    if (int rc = check_tile_grid(who, N, H, W, tiles)) return rc;
    const Sections sec = sections(R, D, true);
    if (int rc = check_workspace(who, workspace_bytes, sec.total)) return rc;
    char* const ws = static_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = forward(c, ws, sec, nullptr, nullptr, skipped, st)) return rc;
    int* const hdr = reinterpret_cast<int*>(ws + sec.hdr);
    const Row* const rows = reinterpret_cast<const Row*>(ws + sec.rows);
    const int* const stat = reinterpret_cast<const int*>(ws + sec.stat);
    const int* const live = reinterpret_cast<const int*>(ws + sec.live);
    double* const stats = reinterpret_cast<double*>(ws + sec.stats);
    const double* const E = reinterpret_cast<const double*>(ws + sec.E);
    const double* const Hh = reinterpret_cast<const double*>(ws + sec.Hh);
    const double* const Z = reinterpret_cast<const double*>(ws + sec.Z);
    const double* const lse = reinterpret_cast<const double*>(ws + sec.lse);
    double* const dZ = reinterpret_cast<double*>(ws + sec.dZ);
    double* const dE = reinterpret_cast<double*>(ws + sec.dE);
    const int chunks = (D + DC - 1) / DC;

    if (grad_W2 || grad_b2) {
        const dim3 grid((unsigned)((K + KT - 1) / KT));
#define CNL_DW2(n_) hipLaunchKernelGGL(dw2_kernel<n_>, grid, dim3(THREADS), 0, st, Z, live, rows, hdr, W2, b2, D, K, lse, scale, grad_W2, grad_b2)
        if (chunks <= 1) CNL_DW2(1); else if (chunks <= 2) CNL_DW2(2); else if (chunks <= 4) CNL_DW2(4); else CNL_DW2(8);
#undef CNL_DW2
        if (int rc = cnl::check_launch("reid_loss dw2_kernel")) return rc;
    }
    if (grad_reid || grad_W1 || grad_gamma || grad_beta) {
        const dim3 grid((unsigned)((R + RB - 1) / RB));
#define CNL_DZ(n_) hipLaunchKernelGGL(dz_kernel<n_>, grid, dim3(THREADS), 0, st, Z, live, rows, hdr, W2, b2, D, K, lse, scale, dZ)
        if (chunks <= 1) CNL_DZ(1); else if (chunks <= 2) CNL_DZ(2); else if (chunks <= 4) CNL_DZ(4); else CNL_DZ(8);
#undef CNL_DZ
        if (int rc = cnl::check_launch("reid_loss dz_kernel")) return rc;
        hipLaunchKernelGGL(bn_grad_kernel, dim3((unsigned)((D + FJ - 1) / FJ)), dim3(THREADS), 0, st, Hh, Z, dZ, live, hdr, D, gamma, stats, grad_gamma, grad_beta);
        if (int rc = cnl::check_launch("reid_loss bn_grad_kernel")) return rc;
    }
    if (grad_reid || grad_W1) {
        hipLaunchKernelGGL(dh_kernel, dim3(blocks_for(R * D)), dim3(THREADS), 0, st, Hh, Z, rows, stats, gamma, hdr, R, D, p->training, dZ);
        if (int rc = cnl::check_launch("reid_loss dh_kernel")) return rc;
    }
    if (grad_W1) {
        const int t = (D + 15) / 16;
        hipLaunchKernelGGL(dw1_kernel, dim3((unsigned)(t * t)), dim3(THREADS), 0, st, dZ, E, stat, hdr, D, grad_W1);
        if (int rc = cnl::check_launch("reid_loss dw1_kernel")) return rc;
    }
    if (grad_reid) {
        hipLaunchKernelGGL(de_kernel, dim3(blocks_for(R * D)), dim3(THREADS), 0, st, dZ, W1, rows, R, D, dE);
        if (int rc = cnl::check_launch("reid_loss de_kernel")) return rc;
        ScatterArgs a;
        a.grad = grad_reid; a.gn = gn; a.gc = gc; a.gh = gh; a.gw = gw;
        a.rows = rows; a.dE = dE; a.D = D; a.H = H; a.W = W; a.Gmax = Gmax; a.tx = tiles_x(W); a.cminor = gc == 1;
        hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)(N * tiles)), dim3(THREADS), 0, st, a);
        if (int rc = cnl::check_launch("reid_loss scatter_kernel")) return rc;
    }
    return CNL_OK;
}
