// lsap_device.h — the assignment solver as device code, shared by track_streams.hip (association of video streams) and mot_eval.hip
// (HOTA / CLEAR / Identity): scipy.optimize.linear_sum_assignment's algorithm in scipy's order and in float64, one wave per problem.
// Include it AFTER the including file's `#pragma clang fp contract(off)`: the reduced costs decide ties exactly as scipy's do.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace cnl_track {

constexpr int LSAP_MAX_SHORT = 1024;     // min(n, T): rows of the (possibly transposed) problem
constexpr int LSAP_MAX_LONG = 4096;      // max(n, T): its columns
// status words (cnl_lsap_batch_f64; cnl_track_streams_f32 adds 16 for the box stage)
constexpr int LSAP_OK = 0, LSAP_INVALID = 1, LSAP_INFEASIBLE = 2, LSAP_TOO_LARGE = 3, STREAM_BAD_TABLE = 4;

// The solver's state, carved from dynamic LDS: 12 bytes per row + 28 bytes per column.
struct LsapLds {
    double *u, *v, *spc;
    int *path, *row4col, *remaining, *col4row;
};
__host__ __device__ inline size_t lsap_lds_bytes(int nr_cap, int nc_cap) { return 12ul * nr_cap + 28ul * nc_cap; }
__device__ __forceinline__ LsapLds lsap_carve(double* base, int nr_cap, int nc_cap) {
    LsapLds L;
    L.u = base;
    L.v = L.u + nr_cap;
    L.spc = L.v + nc_cap;
    L.path = reinterpret_cast<int*>(L.spc + nc_cap);
    L.row4col = L.path + nc_cap;
    L.remaining = L.row4col + nc_cap;
    L.col4row = L.remaining + nc_cap;
    return L;
}

// nr <= nc; C(i, j) = cost[i * rs + j * cs].  Called by the 64 lanes of a single-wave workgroup; every branch on the solver's state is
// uniform.  On LSAP_OK, L.col4row[i] is row i's column and L.row4col[j] column j's row (or -1).
__device__ int lsap_wave(const double* __restrict__ cost, const long rs, const long cs, const int nr, const int nc, const LsapLds L) {
    const int lane = threadIdx.x;
    const double INF = __builtin_inf();
    for (int i = lane; i < nr; i += 64) { L.u[i] = 0.0; L.col4row[i] = -1; }
    for (int j = lane; j < nc; j += 64) { L.v[j] = 0.0; L.row4col[j] = -1; L.path[j] = -1; }
    __syncthreads();
    for (int cur = 0; cur < nr; ++cur) {
        for (int it = lane; it < nc; it += 64) { L.remaining[it] = nc - it - 1; L.spc[it] = INF; }
        __syncthreads();
        double min_val = 0.0;
        int num_remaining = nc, sink = -1, i = cur;
        while (sink == -1) {
            // scipy's scan `for it in 0..num_remaining: ... if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) { lowest = spc[j]; index = it; }`
            // picks, among the columns holding the minimum, the LAST unassigned one if any is unassigned, else the FIRST: the key of this
            // reduction (a lane walks its own positions in ascending order with scipy's very condition, the lanes are merged by the same order).
            double best = INF;
            int best_it = -1, best_free = 0;
            const double ui = L.u[i];
            const double* row = cost + (long)i * rs;
            for (int it = lane; it < num_remaining; it += 64) {
                const int j = L.remaining[it];
                const double r = ((min_val + row[(long)j * cs]) - ui) - L.v[j];
                double sp = L.spc[j];
                if (r < sp) { L.path[j] = i; L.spc[j] = r; sp = r; }
                const int fr = L.row4col[j] == -1;
                if (sp < best || (sp == best && fr)) { best = sp; best_it = it; best_free = fr; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(best_it, o, 64), of = __shfl_xor(best_free, o, 64);
                const bool take = ob < best || (ob == best && (of != best_free ? of : (of ? oi > best_it : oi < best_it)));
                if (take) { best = ob; best_it = oi; best_free = of; }
            }
            min_val = best;
            if (min_val == INF) return LSAP_INFEASIBLE;
            const int j = L.remaining[best_it], last = L.remaining[num_remaining - 1], r4c = L.row4col[j];
            if (r4c == -1) sink = j; else i = r4c;
            --num_remaining;
            __syncthreads();
            // removal is scipy's swap-with-last; the removed column is parked behind the live part, which lists the scanned columns (SC)
            if (lane == 0) { L.remaining[best_it] = last; L.remaining[num_remaining] = j; }
            __syncthreads();
        }
        // dual updates: u[cur] += minVal; u[i] += minVal - spc[col4row[i]] for the other visited rows (the rows of the scanned, assigned
        // columns); v[j] -= minVal - spc[j] for the scanned columns.  Same operands and operations as scipy, distinct addresses per lane.
        if (lane == 0) L.u[cur] = L.u[cur] + min_val;
        for (int idx = num_remaining + lane; idx < nc; idx += 64) {
            const int j = L.remaining[idx];
            const double d = min_val - L.spc[j];
            const int r = L.row4col[j];
            if (r != -1) L.u[r] = L.u[r] + d;
            L.v[j] = L.v[j] - d;
        }
        __syncthreads();
        if (lane == 0) {      // augment along the path (sequential by nature; at most cur + 1 steps)
            int j = sink;
            while (true) {
                const int pi = L.path[j];
                L.row4col[j] = pi;
                const int t = L.col4row[pi];
                L.col4row[pi] = j;
                j = t;
                if (pi == cur) break;
            }
        }
        __syncthreads();
    }
    return LSAP_OK;
}

// One n x T problem (row stride ld) as scipy treats it: invalid entries refused, transposed when n > T, result per ORIGINAL row:
// out[r] = assigned column or -1 (out: global memory or LDS outside L).  Nothing is written unless the status is LSAP_OK.
__device__ int lsap_problem(const double* __restrict__ cost, const long ld, const int n, const int T, const int nr_cap, const int nc_cap,
                            const LsapLds L, int* out) {
    const int lane = threadIdx.x;
    if (n <= 0 || T <= 0) return LSAP_OK;
    const bool transposed = n > T;
    const int nr = transposed ? T : n, nc = transposed ? n : T;
    if (nr > nr_cap || nc > nc_cap) return LSAP_TOO_LARGE;
    int bad = 0;
    for (long p = lane; p < (long)n * T; p += 64) {
        const long r = p / T;
        const double c = cost[r * ld + (p - r * T)];
        bad |= (c != c) || (c == -__builtin_inf());
    }
    if (__ballot(bad) != 0ull) return LSAP_INVALID;
    const int st = transposed ? lsap_wave(cost, 1, ld, nr, nc, L) : lsap_wave(cost, ld, 1, nr, nc, L);
    if (st != LSAP_OK) return st;
    const int* src = transposed ? L.row4col : L.col4row;
    for (int r = lane; r < n; r += 64) out[r] = src[r];
    __syncthreads();
    return LSAP_OK;
}

}  // namespace cnl_track
