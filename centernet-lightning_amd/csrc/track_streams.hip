// track_streams.hip — one association pass for S independent video streams (one frame from each), assignment included.
//
// track.hip leaves the Hungarian step to scipy on the host: per frame the n x T cost matrices cross PCIe and the host thread solves
// them one stream after the other.  Here the matrices stay in a device workspace and the assignment runs on the device, one
// single-wave workgroup per stream, so that S streams are solved on S CUs at once and only the match lists reach the host:
//
//   streams_costs_kernel    compaction + cost matrices of every live stream (the device code of track.hip's frame_kernel, shared
//                           through track_costs.h: bit-identical matrices), written to the workspace; frame record header / detections
//   streams_assign_kernel   per stream: stage 1 (re-ID matrix, cost < reid_threshold), stage 2 (box-cost sub-matrix of what is still
//                           unmatched, cost < box_threshold), match / unmatched lists into the stream's record (mapped host memory)
//   lsap_batch_kernel       the solver alone on B caller-supplied matrices (cnl_lsap_batch_f64)
// cnl_track_streams_low_f32 instantiates both stream kernels with LOW: the cost launch also compacts the low-score detections and writes their
// box costs, the assign kernel runs a third stage (BYTE) on them behind stage 2 — same bodies, same solver, same LDS bound.
// cnl_track_streams_gated_f32 is that entry with a gated cost launch (streams_costs_gated_kernel: class / motion gates inside the per-pair cost
// functions, a gated pair costs CNL_TRACK_GATE_COST); the assign kernel is the same one and never learns of the gates.
//
// The solver is scipy.optimize.linear_sum_assignment's algorithm (rectangular shortest augmenting path, Crouse 2016) in scipy's
// order and in float64, because the RESULT must be scipy's, ties included: box-cost matrices are full of ties (every non-overlapping
// pair costs exactly 1.0) and a different optimal assignment changes which pairs survive the threshold.  What is parallel is the scan
// over the remaining columns (64 lanes) and the dual updates; the augmentations and the steps of a scan are sequential, as there.
#include "track_costs.h"

#pragma clang fp contract(off)   // one rounding per operation: the reduced costs decide ties exactly as scipy's do

#include "lsap_device.h"      // LsapLds, lsap_carve, lsap_wave, lsap_problem and the solver's limits and status words

namespace cnl_track {

__global__ __launch_bounds__(64) void lsap_batch_kernel(const double* __restrict__ cost, const long long* __restrict__ cost_offset,
                                                        const int* __restrict__ row_stride, const int* __restrict__ n_rows,
                                                        const int* __restrict__ n_cols, int* __restrict__ col4row,
                                                        const long long* __restrict__ col4row_offset, int* __restrict__ status,
                                                        int nr_cap, int nc_cap) {
    extern __shared__ double lsap_lds[];
    const int b = blockIdx.x;
    const int n = n_rows[b], T = n_cols[b], ld = row_stride[b];
    int st;
    if (n < 0 || T < 0 || ld < T) st = LSAP_TOO_LARGE;
    else st = lsap_problem(cost + cost_offset[b], ld, n, T, nr_cap, nc_cap, lsap_carve(lsap_lds, nr_cap, nc_cap), col4row + col4row_offset[b]);
    if (threadIdx.x == 0) status[b] = st;
}

// ---------------------------------------------------------------------------------------------------------------- S streams
// Workspace (P = k * R pairs, R = rows of the pooled track table): f64 reid[P] | f64 sub[P] | f32 box[P] | int32 n[S] | col[S][k] |
// ud[S][k] | ut[R] | tflag[R].  Stream s owns pairs k * trk_off[s] ... and rows trk_off[s] ... of ut / tflag.
struct StreamWs {
    double *reid, *sub;
    float* box;
    int *n, *col, *ud, *ut, *tflag;
    float* low_box;     // LOW only: behind everything above, f32 low_box[P] | int32 n_low[S]
    int* n_low;
};
__host__ __device__ inline size_t streams_ws_bytes(long S, long k, long R) { return 20ul * k * R + 4ul * (S + 2 * S * k + 2 * R); }
__host__ __device__ inline size_t streams_low_ws_bytes(long S, long k, long R) { return streams_ws_bytes(S, k, R) + 4ul * k * R + 4ul * S; }
__device__ __forceinline__ StreamWs streams_ws(char* ws, int S, int k, int R, int s, int t0) {
    const long P = (long)k * R;
    StreamWs w;
    w.reid = reinterpret_cast<double*>(ws) + (long)k * t0;
    w.sub = reinterpret_cast<double*>(ws) + P + (long)k * t0;
    w.box = reinterpret_cast<float*>(ws + 16 * P) + (long)k * t0;
    int* ints = reinterpret_cast<int*>(ws + 20 * P);
    w.n = ints + s;
    w.col = ints + S + (long)s * k;
    w.ud = ints + S + (long)S * k + (long)s * k;
    w.ut = ints + S + 2l * S * k + t0;
    w.tflag = w.ut + R;
    char* low = ws + streams_ws_bytes(S, k, R);
    w.low_box = reinterpret_cast<float*>(low) + (long)k * t0;
    w.n_low = reinterpret_cast<int*>(low + 4 * P) + s;
    return w;
}
// Record of one stream: int32 header[16] | det_index[k] | (boxes[k][4] scores[k] labels[k]) | matches[k][2] | unmatched dets[k] | unmatched tracks[T]
// LOW: int32 header[24], and behind the unmatched tracks: low_index[k] | low_matches[k][2]
struct StreamRec {
    int off_index, off_dets, off_match, off_udet, off_utrk, off_low_index, off_low_match;
    long bytes;
};
__host__ __device__ inline StreamRec stream_rec(int k, int T, int with_dets, bool low = false) {
    StreamRec r;
    r.off_index = low ? 96 : 64;
    r.off_dets = (r.off_index + 4 * k + 7) & ~7;
    r.off_match = r.off_dets + (with_dets ? 24 * k : 0);
    r.off_udet = r.off_match + 8 * k;
    r.off_utrk = r.off_udet + 4 * k;
    r.off_low_index = r.off_utrk + 4 * T;
    r.off_low_match = r.off_low_index + 4 * k;
    r.bytes = ((low ? (long)r.off_low_match + 8l * k : (long)r.off_utrk + 4l * T) + 7) & ~7l;
    return r;
}

// grid (pair blocks of the largest stream, S_live): blockIdx.y = slot i of this step's detections, stream live[i].
// GATED (cnl_track_streams_gated_f32): the class / motion gates inside the per-pair cost functions (`g`: the pooled tables); every other byte as LOW.
template <bool LOW, bool GATED>
__device__ __forceinline__ void streams_costs_body(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                   const float* __restrict__ det_score, const void* __restrict__ det_label, int label_kind,
                                                   const int* __restrict__ live, const int* __restrict__ trk_off, int S, int k, int E, float thr,
                                                   float low_thr,
                                                   const float* __restrict__ trk_emb, const float* __restrict__ trk_box, int R, int T_max,
                                                   int box_mode, int reid_metric, int with_dets, char* __restrict__ ws,
                                                   char* __restrict__ record, long record_stride, const GateOps& pooled) {
    __shared__ int sel[MAXK];
    __shared__ int low_sel[LOW ? MAXK : 1];
    __shared__ int wave_sum[4];
    const int i = blockIdx.y, s = live[i];
    if (s < 0 || s >= S) return;                                   // (refused on the host; never index with it)
    const int t0 = trk_off[s], T = trk_off[s + 1] - t0;
    const bool table_ok = t0 >= 0 && T >= 0 && t0 + T <= R && T <= T_max;
    const float* de = det_emb + (long)i * k * E;
    const float* db = det_box + (long)i * k * 4;
    const float* dsc = det_score + (long)i * k;
    const int n = compact_scores(dsc, k, thr, sel, wave_sum);
    const int n_low = LOW ? compact_scores_in<true>(dsc, k, low_thr, thr, low_sel, wave_sum) : 0;
    if (blockIdx.x == 0) {
        const int tid = threadIdx.x;
        char* rec = record + (long)s * record_stride;
        const StreamRec ro = stream_rec(k, T_max, with_dets, LOW);
        int* hdr = reinterpret_cast<int*>(rec);
        if (tid == 0) {
            hdr[0] = n; hdr[1] = k; hdr[2] = T; hdr[4] = ro.off_index; hdr[5] = ro.off_dets; hdr[6] = ro.off_match; hdr[7] = ro.off_udet;
            hdr[8] = ro.off_utrk; hdr[13] = with_dets; hdr[14] = i; hdr[15] = s;
            if (table_ok) *streams_ws(ws, S, k, R, s, t0).n = n;
            if (LOW) {
                hdr[16] = n_low; hdr[18] = ro.off_low_index; hdr[19] = ro.off_low_match; hdr[20] = hdr[21] = hdr[22] = hdr[23] = 0;
                if (table_ok) *streams_ws(ws, S, k, R, s, t0).n_low = n_low;
            }
        }
        if (LOW) {
            int* low_index = reinterpret_cast<int*>(rec + ro.off_low_index);
            for (int q = tid; q < n_low; q += 256) low_index[q] = low_sel[q];
        }
        int* det_index = reinterpret_cast<int*>(rec + ro.off_index);
        for (int q = tid; q < n; q += 256) det_index[q] = sel[q];
        if (with_dets) {
            float* o = reinterpret_cast<float*>(rec + ro.off_dets);
            for (int q = tid; q < 4 * k; q += 256) o[q] = db[q];
            for (int q = tid; q < k; q += 256) o[4 * k + q] = dsc[q];
            int* ol = reinterpret_cast<int*>(o + 5 * k);
            for (int q = tid; q < k; q += 256)
                ol[q] = label_kind == 1 ? (int)(reinterpret_cast<const long long*>(det_label) + (long)i * k)[q]
                      : label_kind == 2 ? (reinterpret_cast<const int*>(det_label) + (long)i * k)[q]
                      : label_kind == 3 ? (int)(reinterpret_cast<const float*>(det_label) + (long)i * k)[q] : 0;
        }
    }
    if (!table_ok) return;
    const StreamWs w = streams_ws(ws, S, k, R, s, t0);
    GateOps g = pooled;       // the stream's rows of the pooled tables, the slot's labels
    if (GATED) {
        if (g.trk_label) g.trk_label += t0;
        if (g.kx) { g.kx += (long)t0 * 8; g.kP += (long)t0 * 64; }
        g.det0 = (long)i * k;
    }
    pair_costs_at<GATED>((long)blockIdx.x * 256 + threadIdx.x, sel, n, de, db, E, trk_emb + (long)t0 * E, trk_box + (long)t0 * 4, T, box_mode, reid_metric,
                         w.reid, w.box, g);
    if (LOW)      // n_low <= k: the grid that covers k * T_max pairs covers these
        pair_box_cost_at<GATED>((long)blockIdx.x * 256 + threadIdx.x, low_sel, n_low, db, trk_box + (long)t0 * 4, T, box_mode, w.low_box, g);
}

template <bool LOW>
__global__ __launch_bounds__(256) void streams_costs_kernel(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                            const float* __restrict__ det_score, const void* __restrict__ det_label, int label_kind,
                                                            const int* __restrict__ live, const int* __restrict__ trk_off, int S, int k, int E, float thr,
                                                            float low_thr,
                                                            const float* __restrict__ trk_emb, const float* __restrict__ trk_box, int R, int T_max,
                                                            int box_mode, int reid_metric, int with_dets, char* __restrict__ ws,
                                                            char* __restrict__ record, long record_stride) {
    streams_costs_body<LOW, false>(det_emb, det_box, det_score, det_label, label_kind, live, trk_off, S, k, E, thr, low_thr, trk_emb, trk_box, R, T_max, box_mode,
                                   reid_metric, with_dets, ws, record, record_stride, GateOps{});
}

__global__ __launch_bounds__(256) void streams_costs_gated_kernel(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                                  const float* __restrict__ det_score, const void* __restrict__ det_label, int label_kind,
                                                                  const int* __restrict__ live, const int* __restrict__ trk_off, int S, int k, int E,
                                                                  float thr, float low_thr, const float* __restrict__ trk_emb,
                                                                  const float* __restrict__ trk_box, int R, int T_max, int box_mode, int reid_metric,
                                                                  int with_dets, char* __restrict__ ws, char* __restrict__ record, long record_stride,
                                                                  GateOps pooled) {
    streams_costs_body<true, true>(det_emb, det_box, det_score, det_label, label_kind, live, trk_off, S, k, E, thr, low_thr, trk_emb, trk_box, R, T_max, box_mode,
                                   reid_metric, with_dets, ws, record, record_stride, pooled);
}

// lanes with `flag` take consecutive positions from `count` on, in lane order (count: uniform, advanced)
__device__ __forceinline__ int wave_pos(const bool flag, int& count) {
    const unsigned long long m = __ballot(flag);
    const int pos = count + __popcll(m & ((1ull << threadIdx.x) - 1ull));
    count += __popcll(m);
    return pos;
}

// One single-wave workgroup per live stream: both assignment stages and the lists of the stream's record.  LOW: then stage 3 — the tracks still
// unmatched that trk_eligible admits (null: all) against the low-score detections, by box cost < low_box_thr; the unmatched-track list is what
// remains after it.
template <bool LOW>
__global__ __launch_bounds__(64) void streams_assign_kernel(const int* __restrict__ live, const int* __restrict__ trk_off, int S, int k, int R, int T_max,
                                                            double reid_thr, float box_thr, float low_box_thr,
                                                            const uint8_t* __restrict__ trk_eligible, int box_mode, int with_dets, char* __restrict__ ws,
                                                            char* __restrict__ record, long record_stride, int nr_cap, int nc_cap) {
    extern __shared__ double lsap_lds[];
    const int lane = threadIdx.x, s = live[blockIdx.x];
    if (s < 0 || s >= S) return;
    char* rec = record + (long)s * record_stride;
    int* hdr = reinterpret_cast<int*>(rec);
    const int t0 = trk_off[s], T = trk_off[s + 1] - t0;
    int status = (t0 >= 0 && T >= 0 && t0 + T <= R) ? (T <= T_max ? LSAP_OK : LSAP_TOO_LARGE) : STREAM_BAD_TABLE;
    const StreamRec ro = stream_rec(k, T_max, with_dets, LOW);
    int* omatch = reinterpret_cast<int*>(rec + ro.off_match);
    int* oud = reinterpret_cast<int*>(rec + ro.off_udet);
    int* out = reinterpret_cast<int*>(rec + ro.off_utrk);
    int m = 0, m1 = 0, nu = 0, tu = 0, m3 = 0;
    if (status == LSAP_OK) {
        const StreamWs w = streams_ws(ws, S, k, R, s, t0);
        const LsapLds L = lsap_carve(lsap_lds, nr_cap, nc_cap);
        const int n = *w.n;
        for (int t = lane; t < T; t += 64) w.tflag[t] = 0;
        status = lsap_problem(w.reid, T, n, T, nr_cap, nc_cap, L, w.col);       // stage 1: the re-ID matrix
        __syncthreads();
        if (status == LSAP_OK) {
            // matches in row order (cost < threshold: float64 against the double, as numpy compares a float64 array with a Python float)
            for (int r0 = 0; r0 < n; r0 += 64) {
                const int r = r0 + lane;
                const bool in = r < n;
                int c = -1;
                bool keep = false;
                if (in && T > 0) {
                    c = w.col[r];
                    keep = c >= 0 && w.reid[(long)r * T + c] < reid_thr;
                }
                const int pos = wave_pos(keep, m);
                if (keep) { omatch[2 * pos] = r; omatch[2 * pos + 1] = c; w.tflag[c] = 1; }
                const int pu = wave_pos(in && !keep, nu);
                if (in && !keep) w.ud[pu] = r;
            }
            m1 = m;
            __syncthreads();
            for (int q0 = 0; q0 < T; q0 += 64) {
                const int t = q0 + lane;
                const bool fr = t < T && !w.tflag[t];
                const int pos = wave_pos(fr, tu);
                if (fr) w.ut[pos] = t;
            }
            __syncthreads();
            bool stage2 = box_mode != 0 && nu > 0 && tu > 0;
            if (stage2) {
                // stage 2: box[np.ix_(unmatched_dets, unmatched_tracks)], which scipy converts to float64
                for (long p = lane; p < (long)nu * tu; p += 64) {
                    const int x = (int)(p / tu), y = (int)(p - (long)x * tu);
                    w.sub[p] = (double)w.box[(long)w.ud[x] * T + w.ut[y]];
                }
                __syncthreads();
                const int st2 = lsap_problem(w.sub, tu, nu, tu, nr_cap, nc_cap, L, w.col);
                __syncthreads();
                if (st2 != LSAP_OK) status = 16 + st2;
                else {
                    int nu2 = 0;
                    for (int x0 = 0; x0 < nu; x0 += 64) {      // float32 cost against the threshold as float32 (numpy's weak-scalar rule)
                        const int x = x0 + lane;
                        const bool in = x < nu;
                        int d = -1, t = -1;
                        bool keep = false;
                        if (in) {
                            d = w.ud[x];
                            const int c = w.col[x];
                            if (c >= 0) { t = w.ut[c]; keep = w.box[(long)d * T + t] < box_thr; }
                        }
                        const int pos = wave_pos(keep, m);
                        if (keep) { omatch[2 * pos] = d; omatch[2 * pos + 1] = t; w.tflag[t] = 1; }
                        const int pu = wave_pos(in && !keep, nu2);
                        if (in && !keep) oud[pu] = d;
                    }
                    nu = nu2;
                }
            } else {
                for (int x = lane; x < nu; x += 64) oud[x] = w.ud[x];
            }
            __syncthreads();
            if (LOW && status == LSAP_OK) {
                // stage 3: low_box[:, U] for U = the eligible tracks still unmatched (ascending), converted to float64 as scipy does
                const int n_low = *w.n_low;
                int n3 = 0;
                for (int q0 = 0; q0 < T; q0 += 64) {
                    const int t = q0 + lane;
                    const bool fr = t < T && !w.tflag[t] && (trk_eligible == nullptr || trk_eligible[t0 + t] != 0);
                    const int pos = wave_pos(fr, n3);
                    if (fr) w.ut[pos] = t;
                }
                __syncthreads();
                if (n_low > 0 && n3 > 0) {
                    for (long p = lane; p < (long)n_low * n3; p += 64) {
                        const int x = (int)(p / n3), y = (int)(p - (long)x * n3);
                        w.sub[p] = (double)w.low_box[(long)x * T + w.ut[y]];
                    }
                    __syncthreads();
                    const int st3 = lsap_problem(w.sub, n3, n_low, n3, nr_cap, nc_cap, L, w.col);
                    __syncthreads();
                    if (st3 != LSAP_OK) status = 32 + st3;
                    else {
                        int* olow = reinterpret_cast<int*>(rec + ro.off_low_match);
                        for (int x0 = 0; x0 < n_low; x0 += 64) {      // float32 cost against the threshold as float32, as in stage 2
                            const int x = x0 + lane;
                            int t = -1;
                            bool keep = false;
                            if (x < n_low) {
                                const int c = w.col[x];
                                if (c >= 0) { t = w.ut[c]; keep = w.low_box[(long)x * T + t] < low_box_thr; }
                            }
                            const int pos = wave_pos(keep, m3);
                            if (keep) { olow[2 * pos] = x; olow[2 * pos + 1] = t; w.tflag[t] = 1; }
                        }
                    }
                    __syncthreads();
                }
            }
            tu = 0;
            if (status == LSAP_OK)
                for (int q0 = 0; q0 < T; q0 += 64) {
                    const int t = q0 + lane;
                    const bool fr = t < T && !w.tflag[t];
                    const int pos = wave_pos(fr, tu);
                    if (fr) out[pos] = t;
                }
        }
    }
    if (lane == 0) {
        const bool ok = status == LSAP_OK;
        hdr[3] = status; hdr[9] = ok ? m : 0; hdr[10] = ok ? m1 : 0; hdr[11] = ok ? nu : 0; hdr[12] = ok ? tu : 0;
        if (LOW) hdr[17] = ok ? m3 : 0;
    }
}

static cnl::DeviceOnce lsap_once, assign_once, assign_low_once;
constexpr int LSAP_LDS_MAX = 12 * LSAP_MAX_SHORT + 28 * LSAP_MAX_LONG;      // 126976 of the CU's 160 KiB

}  // namespace cnl_track
using namespace cnl_track;

extern "C" int cnl_lsap_batch_f64(const double* cost, const int64_t* cost_offset, const int32_t* row_stride, const int32_t* n_rows,
                                  const int32_t* n_cols, int32_t B, int32_t max_rows, int32_t max_cols, int32_t* col4row,
                                  const int64_t* col4row_offset, int32_t* status, void* stream) {
    CNL_REQUIRE(B >= 0 && max_rows >= 0 && max_cols >= 0, CNL_E_BAD_ARG, "cnl_lsap_batch_f64: negative B / max_rows / max_cols");
    if (B == 0) return CNL_OK;
    CNL_REQUIRE(cost && cost_offset && row_stride && n_rows && n_cols && col4row && col4row_offset && status, CNL_E_BAD_ARG,
                "cnl_lsap_batch_f64: null pointer");
    const int lo = max_rows < max_cols ? max_rows : max_cols, hi = max_rows < max_cols ? max_cols : max_rows;
    CNL_REQUIRE(lo <= LSAP_MAX_SHORT && hi <= LSAP_MAX_LONG, CNL_E_UNSUPPORTED,
                "cnl_lsap_batch_f64: problems of up to %d x %d: min(rows, cols) <= %d and max(rows, cols) <= %d are supported", max_rows, max_cols,
                LSAP_MAX_SHORT, LSAP_MAX_LONG);
    const int nr_cap = lo > 0 ? lo : 1, nc_cap = hi > 0 ? hi : 1;
    if (int rc = cnl::kernel_setup(lsap_once, (const void*)lsap_batch_kernel, LSAP_LDS_MAX)) return rc;
    hipLaunchKernelGGL(lsap_batch_kernel, dim3((unsigned)B), dim3(64), lsap_lds_bytes(nr_cap, nc_cap), (hipStream_t)stream, cost,
                       (const long long*)cost_offset, row_stride, n_rows, n_cols, col4row, (const long long*)col4row_offset, status, nr_cap, nc_cap);
    return cnl::check_launch("lsap_batch_kernel");
}

extern "C" int64_t cnl_track_streams_workspace_bytes(int32_t S, int32_t k, int32_t T_max) {
    if (S <= 0 || k <= 0 || T_max < 0) return 0;
    return (int64_t)streams_ws_bytes(S, k, (long)S * T_max);
}

extern "C" int64_t cnl_track_streams_record_bytes(int32_t k, int32_t T_max, int32_t with_detections) {
    if (k <= 0 || T_max < 0) return 0;
    return stream_rec(k, T_max, with_detections ? 1 : 0).bytes;
}

extern "C" int64_t cnl_track_streams_low_workspace_bytes(int32_t S, int32_t k, int32_t T_max) {
    if (S <= 0 || k <= 0 || T_max < 0) return 0;
    return (int64_t)streams_low_ws_bytes(S, k, (long)S * T_max);
}

extern "C" int64_t cnl_track_streams_low_record_bytes(int32_t k, int32_t T_max, int32_t with_detections) {
    if (k <= 0 || T_max < 0) return 0;
    return stream_rec(k, T_max, with_detections ? 1 : 0, true).bytes;
}

// cnl_track_streams_f32 (low = false; the three low arguments unused), cnl_track_streams_low_f32 and cnl_track_streams_gated_f32 (low, gate set: its
// cost launch is the gated one, and without a low-score stage — low_threshold == detection_threshold — it also takes box_cost 0): one set of checks,
// the same assign launch.
static int streams_launch(const char* name, bool low, const cnl_track_gate* gate, const float* det_emb, const float* det_box, const float* det_score, const void* det_label,
                          int32_t label_kind, int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                          double reid_threshold, float box_threshold, float low_threshold, float low_box_threshold, const float* trk_emb,
                          const float* trk_box, const int32_t* trk_off, const uint8_t* trk_eligible, int32_t R, int32_t T_max, int32_t box_cost,
                          int32_t reid_metric, int32_t with_detections, void* workspace, int64_t workspace_bytes, void* record, int64_t record_stride,
                          void* stream) {
    CNL_REQUIRE(det_emb && det_box && det_score && live && trk_off && workspace && record, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(S > 0 && S_live > 0 && S_live <= S && k > 0 && E > 0 && R >= 0 && T_max >= 0, CNL_E_BAD_ARG,
                "%s: bad S / S_live / k / E / R / T_max (%d / %d / %d / %d / %d / %d)", name, S, S_live, k, E, R, T_max);
    CNL_REQUIRE(k <= MAXK, CNL_E_UNSUPPORTED, "%s: k = %d > %d detections per frame", name, k, MAXK);
    CNL_REQUIRE(T_max <= LSAP_MAX_LONG, CNL_E_UNSUPPORTED, "%s: T_max = %d > %d tracks per stream", name, T_max, LSAP_MAX_LONG);
    CNL_REQUIRE(S_live <= 65535, CNL_E_UNSUPPORTED, "%s: S_live = %d > 65535 streams per step", name, S_live);
    const bool low_stage = low && !(gate != nullptr && low_threshold == detection_threshold);
    CNL_REQUIRE(box_cost >= (low_stage ? 1 : 0) && box_cost <= 2, CNL_E_BAD_ARG, "%s: box_cost must be %s1 (iou), 2 (giou)", name, low_stage ? "" : "0 (none), ");
    CNL_REQUIRE(!low || (low_threshold >= 0.f && low_threshold <= detection_threshold), CNL_E_BAD_ARG,
                "%s: low_threshold %g must lie in [0, detection_threshold = %g]", name, (double)low_threshold, (double)detection_threshold);
    CNL_REQUIRE(reid_metric >= 0 && reid_metric <= 7, CNL_E_BAD_ARG, "%s: reid_metric must be 0 (cosine) .. 7 (correlation)", name);
    CNL_REQUIRE(label_kind >= 0 && label_kind <= 3 && (label_kind == 0 || det_label), CNL_E_BAD_ARG,
                "%s: label_kind must be 0 (none), 1 (int64), 2 (int32), 3 (float32) with det_label set", name);
    if (int rc = check_gate(name, gate, det_box, {reid_threshold, (double)box_threshold, (double)low_box_threshold})) return rc;
    CNL_REQUIRE(R == 0 || trk_emb, CNL_E_BAD_ARG, "%s: R > 0 without track table", name);
    CNL_REQUIRE(R == 0 || box_cost == 0 || trk_box, CNL_E_BAD_ARG, "%s: box cost requested without track boxes", name);
    CNL_REQUIRE(((uintptr_t)record & 7) == 0 && ((uintptr_t)workspace & 7) == 0 && (record_stride & 7) == 0, CNL_E_BAD_ARG,
                "%s: record, record_stride and workspace must be 8-byte aligned", name);
    CNL_REQUIRE(inputs_aligned(det_emb, det_box, trk_emb, trk_box, E, R, box_cost), CNL_E_BAD_ARG, "%s: %s", name, INPUTS_ALIGNED);
    const int wd = with_detections ? 1 : 0;
    const int64_t rec_need = stream_rec(k, T_max, wd, low).bytes, ws_need = (int64_t)(low ? streams_low_ws_bytes(S, k, R) : streams_ws_bytes(S, k, R));
    CNL_REQUIRE(record_stride >= rec_need, CNL_E_BAD_ARG, "%s: record_stride %ld, k = %d, T_max = %d needs %ld (cnl_track_streams%s_record_bytes)", name,
                (long)record_stride, k, T_max, (long)rec_need, low ? "_low" : "");
    CNL_REQUIRE(workspace_bytes >= ws_need, CNL_E_BAD_ARG, "%s: workspace holds %ld bytes, S = %d, k = %d, R = %d needs %ld", name, (long)workspace_bytes, S,
                k, R, (long)ws_need);
    const int lo = k < T_max ? k : T_max, hi = k < T_max ? T_max : k;
    const int nr_cap = lo > 0 ? lo : 1, nc_cap = hi;
    if (int rc = low ? cnl::kernel_setup(assign_low_once, (const void*)streams_assign_kernel<true>, LSAP_LDS_MAX)
                     : cnl::kernel_setup(assign_once, (const void*)streams_assign_kernel<false>, LSAP_LDS_MAX))
        return rc;
    const long pairs = (long)k * T_max;
    const unsigned gx = (unsigned)(pairs > 0 ? (pairs + 255) / 256 : 1);
    if (gate != nullptr) {
        const GateOps g{gate->trk_label, gate->kx, gate->kP, gate->motion_gate, gate->motion_weight, det_label, label_kind, 0};
        hipLaunchKernelGGL(streams_costs_gated_kernel, dim3(gx, (unsigned)S_live), dim3(256), 0, (hipStream_t)stream, det_emb, det_box, det_score, det_label,
                           label_kind, live, trk_off, S, k, E, detection_threshold, low_threshold, trk_emb, trk_box, R, T_max, box_cost, reid_metric, wd,
                           (char*)workspace, (char*)record, (long)record_stride, g);
    } else
        hipLaunchKernelGGL(low ? streams_costs_kernel<true> : streams_costs_kernel<false>, dim3(gx, (unsigned)S_live), dim3(256), 0, (hipStream_t)stream,
                           det_emb, det_box, det_score, det_label, label_kind, live, trk_off, S, k, E, detection_threshold, low_threshold, trk_emb, trk_box, R,
                           T_max, box_cost, reid_metric, wd, (char*)workspace, (char*)record, (long)record_stride);
    if (int rc = cnl::check_launch("track streams_costs_kernel")) return rc;
    hipLaunchKernelGGL(low ? streams_assign_kernel<true> : streams_assign_kernel<false>, dim3((unsigned)S_live), dim3(64), lsap_lds_bytes(nr_cap, nc_cap),
                       (hipStream_t)stream, live, trk_off, S, k, R, T_max, reid_threshold, box_threshold, low_box_threshold, trk_eligible, box_cost, wd,
                       (char*)workspace, (char*)record, (long)record_stride, nr_cap, nc_cap);
    return cnl::check_launch("track streams_assign_kernel");
}

extern "C" int cnl_track_streams_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                     int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                                     double reid_threshold, float box_threshold, const float* trk_emb, const float* trk_box,
                                     const int32_t* trk_off, int32_t R, int32_t T_max, int32_t box_cost, int32_t reid_metric,
                                     int32_t with_detections, void* workspace, int64_t workspace_bytes, void* record, int64_t record_stride,
                                     void* stream) {
    return streams_launch("cnl_track_streams_f32", false, nullptr, det_emb, det_box, det_score, det_label, label_kind, S, S_live, live, k, E, detection_threshold,
                          reid_threshold, box_threshold, 0.f, 0.f, trk_emb, trk_box, trk_off, nullptr, R, T_max, box_cost, reid_metric, with_detections,
                          workspace, workspace_bytes, record, record_stride, stream);
}

extern "C" int cnl_track_streams_low_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                         int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                                         double reid_threshold, float box_threshold, float low_threshold, float low_box_threshold,
                                         const float* trk_emb, const float* trk_box, const int32_t* trk_off, const uint8_t* trk_eligible, int32_t R,
                                         int32_t T_max, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* workspace,
                                         int64_t workspace_bytes, void* record, int64_t record_stride, void* stream) {
    return streams_launch("cnl_track_streams_low_f32", true, nullptr, det_emb, det_box, det_score, det_label, label_kind, S, S_live, live, k, E,
                          detection_threshold, reid_threshold, box_threshold, low_threshold, low_box_threshold, trk_emb, trk_box, trk_off, trk_eligible, R,
                          T_max, box_cost, reid_metric, with_detections, workspace, workspace_bytes, record, record_stride, stream);
}

extern "C" int cnl_track_streams_gated_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                           int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                                           double reid_threshold, float box_threshold, float low_threshold, float low_box_threshold,
                                           const float* trk_emb, const float* trk_box, const int32_t* trk_off, const uint8_t* trk_eligible, int32_t R,
                                           int32_t T_max, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* workspace,
                                           int64_t workspace_bytes, void* record, int64_t record_stride, const cnl_track_gate* gate, void* stream) {
    static const cnl_track_gate off = {nullptr, nullptr, nullptr, 0.0, 1.0};
    return streams_launch("cnl_track_streams_gated_f32", true, gate ? gate : &off, det_emb, det_box, det_score, det_label, label_kind, S, S_live, live, k, E,
                          detection_threshold, reid_threshold, box_threshold, low_threshold, low_box_threshold, trk_emb, trk_box, trk_off, trk_eligible, R,
                          T_max, box_cost, reid_metric, with_detections, workspace, workspace_bytes, record, record_stride, stream);
}
