// track_lifecycle.hip — the track life cycle of a TrackerBank step on the device (include/centernet_gfx950.h: cnl_track_lifecycle_i32,
// cnl_track_lifecycle_emit_f64), so that a step is a fixed sequence of launches and the host neither reads a match list nor keeps a Track.
//
// track_streams.hip leaves the state machine of centernet_lightning/models/tracker.py:164-196, 305-347 (Track.update / mark_missed, the births,
// the deletions, the id counter) to Python: the host waits for the records, walks them per track and writes the index lists of the table
// update.  Here the records stay in device memory and three kernels do that work between the assign launch and the end of the step:
//
//   lifecycle_kernel   one single-wave workgroup per stream: the stream's record -> the new state of its old rows, the survivors compacted in
//                      row order, the births behind them, the id counter, the sticky status word; into a staging section of max_tracks rows
//   pack_kernel        prefix sum of the streams' new counts -> the new trk_off; staging -> the pooled row arrays and the global index lists
//                      (src_trk / src_det / keep_emb / flags) that cnl_track_apply_keep_f32 and cnl_track_kalman_f64 read UNCHANGED, over the
//                      capacity: a padding row carries itself
//   emit_kernel        behind the table update (and the filter): the reported box of every row, and the ACTIVE rows of every participating
//                      slot compacted into the step's output tensors
// No allocation, no synchronisation, no atomics: every word has one writer, so every run gives the same bits.  tests/lifecycle_ref.py restates
// the three kernels in numpy and is held equal to the host path's life_cycle + Track.
#include "cnl_common.h"
#include "lsap_device.h"      // LSAP_MAX_LONG: the assign kernel's bound on the tracks of one stream

namespace cnl_lifecycle {

constexpr int MAX_TRACKS = cnl_track::LSAP_MAX_LONG;        // rows of one stream
constexpr int MAX_STREAMS = 4096;               // pack_kernel keeps the S + 1 offsets in LDS
// TrackState of the host path (enum.auto: 1 ..)
constexpr int UNCONFIRMED = 1, ACTIVE = 2, INACTIVE = 3, TO_DELETE = 4;
constexpr int BAD_RECORD = cnl_track::STREAM_BAD_TABLE;     // a record whose sections do not lie inside record_stride: treated as a skipped stream

using Args = cnl_track_lifecycle;

// staging of stream s: max_tracks rows from row s * max_tracks on.  workspace: int64 id[C] | int32 src_trk[C] | src_det[C] | keep[C] | state[C] |
// birth_age[C] | inactive_age[C] | label[C] | count[S] | part[S]   (C = S * max_tracks)
struct Stage {
    long long* id;
    int *src_trk, *src_det, *keep, *state, *birth, *inact, *label, *count, *part;
};
__host__ __device__ inline long stage_bytes(long S, long M) { return 36l * S * M + 8l * S; }
__device__ __forceinline__ Stage stage_of(const Args& a) {
    const long C = (long)a.S * a.max_tracks;
    Stage w;
    w.id = reinterpret_cast<long long*>(a.workspace);
    int* q = reinterpret_cast<int*>(w.id + C);
    w.src_trk = q; w.src_det = q + C; w.keep = q + 2 * C; w.state = q + 3 * C; w.birth = q + 4 * C; w.inact = q + 5 * C; w.label = q + 6 * C;
    w.count = q + 7 * C; w.part = w.count + a.S;
    return w;
}

// lanes with `flag` take consecutive positions from `count` on, in lane order (count: uniform, advanced)
__device__ __forceinline__ int wave_pos(const bool flag, int& count) {
    const unsigned long long m = __ballot(flag);
    const int pos = count + __popcll(m & ((1ull << threadIdx.x) - 1ull));
    count += __popcll(m);
    return pos;
}

__device__ __forceinline__ int label_at(const void* det_label, int label_kind, long g) {      // as the record's label section is cast
    return label_kind == 1 ? (int)reinterpret_cast<const long long*>(det_label)[g]
         : label_kind == 2 ? reinterpret_cast<const int*>(det_label)[g]
         : label_kind == 3 ? (int)reinterpret_cast<const float*>(det_label)[g] : 0;
}

__global__ __launch_bounds__(64) void lifecycle_kernel(const Args a) {
    __shared__ int det_of[MAX_TRACKS];              // per old row: the detection (position in the slot's arrays) that updates it, -1: unmatched
    __shared__ unsigned char keepf[MAX_TRACKS];     // ... and 1 if that was a low-score match
    const int s = blockIdx.x, lane = threadIdx.x, M = a.max_tracks, k = a.k;
    const long base = (long)s * M;
    const Stage w = stage_of(a);
    const int t0 = a.old_rows.trk_off[s];
    int T = a.old_rows.trk_off[s + 1] - t0;
    if (t0 < 0 || T < 0 || T > M || (long)t0 + T > (long)a.S * M) T = 0;      // (pack_kernel never writes such offsets)
    const int slot = a.slot_of[s];
    long long next_id = a.next_track_id[s];
    int count = 0, part = 0, code = 0;
    if (s == a.reset_stream) {          // forgotten: no rows, the counter starts again
        next_id = 0;
    } else {
        const char* rec = reinterpret_cast<const char*>(a.record) + (long)s * a.record_stride;
        const int* hdr = reinterpret_cast<const int*>(rec);
        const bool in_step = slot >= 0 && slot < a.S_live;
        if (in_step) {
            code = hdr[3] != 0 ? (hdr[3] & 0xffff) : 0;
            // the sections this kernel reads (their offsets are the cost kernel's, read from device memory: never index past the record with them)
            const long lim = a.record_stride;
            bool ok = hdr[1] == k && hdr[4] >= 0 && hdr[4] + 4l * k <= lim && hdr[6] >= 0 && hdr[6] + 8l * k <= lim && hdr[7] >= 0 && hdr[7] + 4l * k <= lim;
            if (a.low_record) ok = ok && hdr[18] >= 0 && hdr[18] + 4l * k <= lim && hdr[19] >= 0 && hdr[19] + 8l * k <= lim;
            if (!ok && code == 0) code = BAD_RECORD;
        }
        if (!in_step || code != 0) {
            // no part in this step (or skipped: the association has no valid lists): the rows are carried, nothing ages, nothing predicts
            for (int r = lane; r < T; r += 64) {
                w.id[base + r] = a.old_rows.track_id[t0 + r];
                w.src_trk[base + r] = t0 + r; w.src_det[base + r] = -1; w.keep[base + r] = 0;
                w.state[base + r] = a.old_rows.state[t0 + r]; w.birth[base + r] = a.old_rows.birth_age[t0 + r];
                w.inact[base + r] = a.old_rows.inactive_age[t0 + r]; w.label[base + r] = a.old_rows.label[t0 + r];
            }
            count = T;
        } else {
            for (int r = lane; r < T; r += 64) { det_of[r] = -1; keepf[r] = 0; }
            __syncthreads();
            // stage 1 / 2 matches (detection row, track): the reference quirk — the track is updated from POSITION `row` of the unfiltered arrays
            int m = hdr[9];
            m = m < 0 ? 0 : m > k ? k : m;
            const int* match = reinterpret_cast<const int*>(rec + hdr[6]);
            for (int q = lane; q < m; q += 64) {
                const int d = match[2 * q], t = match[2 * q + 1];
                if ((unsigned)t < (unsigned)T && (unsigned)d < (unsigned)k) det_of[t] = d;
            }
            if (a.low_record) {     // stage 3 matches (low row, track): the ORIGINAL index, no quirk; the embedding is kept
                int m3 = hdr[17];
                m3 = m3 < 0 ? 0 : m3 > k ? k : m3;
                const int* low_index = reinterpret_cast<const int*>(rec + hdr[18]);
                const int* low_match = reinterpret_cast<const int*>(rec + hdr[19]);
                for (int q = lane; q < m3; q += 64) {
                    const int x = low_match[2 * q], t = low_match[2 * q + 1];
                    if ((unsigned)t < (unsigned)T && (unsigned)x < (unsigned)k) {
                        const int d = low_index[x];
                        if ((unsigned)d < (unsigned)k) { det_of[t] = d; keepf[t] = 1; }
                    }
                }
            }
            __syncthreads();
            for (int r0 = 0; r0 < T; r0 += 64) {
                const int r = r0 + lane;
                const bool in = r < T;
                int st = TO_DELETE, birth = 0, inact = 0, d = -1;
                if (in) {
                    st = a.old_rows.state[t0 + r]; birth = a.old_rows.birth_age[t0 + r]; inact = a.old_rows.inactive_age[t0 + r];
                    d = det_of[r];
                    if (d >= 0) {                   // Track.update_matched
                        if (st == UNCONFIRMED) {
                            birth += 1;
                            if (birth >= a.min_birth_age) st = ACTIVE;
                        } else if (st == INACTIVE) { st = ACTIVE; inact = 0; }
                    } else {                        // Track.update_unmatched
                        if (st == UNCONFIRMED) st = TO_DELETE;
                        else if (st == ACTIVE) { st = INACTIVE; inact = 0; }
                        else if (st == INACTIVE) {
                            inact += 1;
                            if (inact >= a.max_inactive_age) st = TO_DELETE;
                        }
                    }
                }
                const bool alive = in && st != TO_DELETE;
                const int pos = wave_pos(alive, count);
                if (alive) {
                    w.id[base + pos] = a.old_rows.track_id[t0 + r];
                    w.src_trk[base + pos] = t0 + r; w.src_det[base + pos] = d >= 0 ? slot * k + d : -1; w.keep[base + pos] = d >= 0 ? keepf[r] : 0;
                    w.state[base + pos] = st; w.birth[base + pos] = birth; w.inact[base + pos] = inact; w.label[base + pos] = a.old_rows.label[t0 + r];
                }
            }
            // births: the unmatched detection rows ascending, the first to be born first; what does not fit into max_tracks rows is dropped
            int nud = hdr[11];
            nud = nud < 0 ? 0 : nud > k ? k : nud;
            const int room = M - count, nb = nud < room ? nud : room;
            if (nud > room) code = 1 << 16;
            const int* udet = reinterpret_cast<const int*>(rec + hdr[7]);
            const int* det_index = reinterpret_cast<const int*>(rec + hdr[4]);
            for (int q = lane; q < nb; q += 64) {
                const int row = udet[q];
                int src = (unsigned)row < (unsigned)k ? det_index[row] : 0;
                if ((unsigned)src >= (unsigned)k) src = 0;
                const long p = base + count + q;
                w.id[p] = next_id + q;
                w.src_trk[p] = -1; w.src_det[p] = slot * k + src; w.keep[p] = 0;
                w.state[p] = UNCONFIRMED; w.birth[p] = 0; w.inact[p] = 0; w.label[p] = label_at(a.det_label, a.label_kind, (long)slot * k + src);
            }
            count += nb;
            next_id += nb;
            part = 1;
        }
    }
    if (lane == 0) {
        w.count[s] = count;
        w.part[s] = part;
        a.next_track_id[s] = next_id;
        if (code != 0) {    // sticky: the first association code and the step of the first event stay; the overflow bit is or-ed in
            int* word = a.status + 2 * s;
            const int have = word[0];
            if (have == 0) word[1] = a.step;
            word[0] = have | (code & (1 << 16)) | ((have & 0xffff) == 0 ? (code & 0xffff) : 0);
        }
    }
}

__global__ __launch_bounds__(256) void pack_kernel(const Args a) {
    __shared__ int off[MAX_STREAMS + 1];
    const Stage w = stage_of(a);
    const int S = a.S, M = a.max_tracks;
    if (threadIdx.x < 64) {       // exclusive prefix sum of the S counts, 64 at a time, by the first wave
        const int lane = threadIdx.x;
        int run = 0;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const int c = s < S ? w.count[s] : 0;
            int inc = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(inc, o, 64);
                if (lane >= o) inc += v;
            }
            if (s < S) off[s] = run + inc - c;
            run += __shfl(inc, 63, 64);
        }
        if (lane == 0) off[S] = run;
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int s = threadIdx.x; s <= S; s += 256) a.new_rows.trk_off[s] = off[s];
    const long C = (long)S * M;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= C) return;
    if (r >= off[S]) {      // padding up to the capacity: the row carries itself through the table update and the filter
        a.src_trk[r] = (int)r; a.src_det[r] = -1; a.keep_emb[r] = 0; a.flags[r] = 0; a.trk_eligible[r] = 0;
        a.new_rows.track_id[r] = 0; a.new_rows.state[r] = 0; a.new_rows.birth_age[r] = 0; a.new_rows.inactive_age[r] = 0; a.new_rows.label[r] = 0;
        return;
    }
    int lo = 0, hi = S;     // the stream of row r: the last s with off[s] <= r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    const long p = (long)lo * M + (r - off[lo]);
    const int st = w.state[p];
    a.src_trk[r] = w.src_trk[p]; a.src_det[r] = w.src_det[p]; a.keep_emb[r] = (unsigned char)w.keep[p]; a.flags[r] = w.part[lo];
    a.trk_eligible[r] = st == ACTIVE;       // the next step's low-score stage: ACTIVE at its start
    a.new_rows.track_id[r] = w.id[p]; a.new_rows.state[r] = st; a.new_rows.birth_age[r] = w.birth[p]; a.new_rows.inactive_age[r] = w.inact[p];
    a.new_rows.label[r] = w.label[p];
}

// the reported box of new row r: a born / matched row's is the detection's (the filter launch's out_box with one), a carried row keeps its own
__device__ __forceinline__ void reported_box(const Args& a, long r, int rows, double (&b)[4]) {
    b[0] = b[1] = b[2] = b[3] = 0.0;
    if (r >= rows) return;
    const int d = a.src_det[r], t = a.src_trk[r];
    if (d >= 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = a.kalman_box ? a.kalman_box[r * 4 + j] : (double)a.det_box[(long)d * 4 + j];
    } else if (t >= 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = a.old_rows.box[(long)t * 4 + j];
    }
}

// blocks 0 .. S_live - 1: the output of slot i; the others: 64 rows of the reported-box array each
__global__ __launch_bounds__(64) void emit_kernel(const Args a) {
    const int lane = threadIdx.x, S = a.S, M = a.max_tracks;
    const int rows = a.new_rows.trk_off[S];
    double b[4];
    if ((int)blockIdx.x >= a.S_live) {
        const long r = ((long)blockIdx.x - a.S_live) * 64 + lane;
        if (r >= (long)S * M) return;
        reported_box(a, r, rows, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) a.new_rows.box[r * 4 + j] = b[j];
        return;
    }
    const int i = blockIdx.x, s = a.live[i];
    if (s < 0 || s >= S) return;
    const int n0 = a.new_rows.trk_off[s], n = a.new_rows.trk_off[s + 1] - n0;
    const long o = (long)i * M;
    int count = 0;
    for (int r0 = 0; r0 < n; r0 += 64) {
        const int r = r0 + lane;
        const bool act = r < n && a.new_rows.state[n0 + r] == ACTIVE;
        const int pos = wave_pos(act, count);
        if (act) {
            reported_box(a, n0 + r, rows, b);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (a.out_box_f64) reinterpret_cast<double*>(a.out_box)[(o + pos) * 4 + j] = b[j];
                else reinterpret_cast<float*>(a.out_box)[(o + pos) * 4 + j] = (float)b[j];
            }
            a.out_track_id[o + pos] = a.new_rows.track_id[n0 + r];
            a.out_label[o + pos] = (long long)a.new_rows.label[n0 + r];
        }
    }
    for (int q = count + lane; q < M; q += 64) {        // slots at and beyond count are zero
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (a.out_box_f64) reinterpret_cast<double*>(a.out_box)[(o + q) * 4 + j] = 0.0;
            else reinterpret_cast<float*>(a.out_box)[(o + q) * 4 + j] = 0.f;
        }
        a.out_track_id[o + q] = 0;
        a.out_label[o + q] = 0;
    }
    if (lane == 0) a.out_count[i] = count;
}

// camera-motion compensation: one single-wave workgroup per slot adds the slot's shift to every position its stream's rows hold
constexpr int BAD_SHIFT = 1 << 17;
__global__ __launch_bounds__(64) void shift_kernel(float* __restrict__ trk_box, double* __restrict__ box, double* __restrict__ kx,
                                                    const int* __restrict__ trk_off, const int* __restrict__ live, const float* __restrict__ shift,
                                                    int* __restrict__ status, int S, int max_tracks, int step) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int s = live[i];
    if (s < 0 || s >= S) return;
    const float dx = shift[2 * i], dy = shift[2 * i + 1];
    if (!(isfinite(dx) && isfinite(dy))) {      // the stream is skipped; sticky, as the life cycle's codes
        if (lane == 0) {
            int* word = status + 2 * s;
            const int have = word[0];
            if (have == 0) word[1] = step;
            word[0] = have | BAD_SHIFT;
        }
        return;
    }
    const int t0 = trk_off[s], t1 = trk_off[s + 1];
    if (t0 < 0 || t1 < t0 || (long)t1 > (long)S * max_tracks) return;
    // item q: coordinate q & 3 of row t0 + (q >> 2); x for even coordinates, y for odd ones
    for (long q = (long)t0 * 4 + lane; q < (long)t1 * 4; q += 64) {
        const float df = (q & 1) ? dy : dx;
        trk_box[q] += df;
        box[q] += (double)df;
        if (kx) kx[(q >> 2) * 8 + (q & 3)] += (double)df;
    }
}

static bool rows_ok(const cnl_track_rows& r) {
    return r.track_id && r.state && r.birth_age && r.inactive_age && r.label && r.box && r.trk_off &&
           (((uintptr_t)r.track_id | (uintptr_t)r.box) & 7) == 0 &&
           (((uintptr_t)r.state | (uintptr_t)r.birth_age | (uintptr_t)r.inactive_age | (uintptr_t)r.label | (uintptr_t)r.trk_off) & 3) == 0;
}

// the checks both entries share
static int check_args(const char* name, const Args* p) {
    CNL_REQUIRE(p, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(p->S > 0 && p->S_live >= 0 && p->S_live <= p->S && p->k > 0 && p->max_tracks > 0, CNL_E_BAD_ARG,
                "%s: bad S / S_live / k / max_tracks (%d / %d / %d / %d)", name, p->S, p->S_live, p->k, p->max_tracks);
    CNL_REQUIRE(p->max_tracks <= MAX_TRACKS, CNL_E_UNSUPPORTED, "%s: max_tracks = %d > %d tracks per stream (the assignment's limit)", name,
                p->max_tracks, MAX_TRACKS);
    CNL_REQUIRE(p->S <= MAX_STREAMS && (long)p->S_live * p->k < (1l << 31), CNL_E_UNSUPPORTED, "%s: S = %d > %d streams, or S_live * k = %ld beyond int32",
                name, p->S, MAX_STREAMS, (long)p->S_live * p->k);      // (so S * max_tracks <= 2^24 rows: int32 row indices)
    CNL_REQUIRE(p->live || p->S_live == 0, CNL_E_BAD_ARG, "%s: null pointer (live)", name);
    CNL_REQUIRE(p->src_trk && p->src_det && p->flags && p->keep_emb && p->trk_eligible && p->workspace, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(rows_ok(p->old_rows) && rows_ok(p->new_rows), CNL_E_BAD_ARG,
                "%s: null pointer in old_rows / new_rows, or track_id / box not 8-byte aligned, or an int32 array not 4-byte aligned", name);
    CNL_REQUIRE(p->old_rows.track_id != p->new_rows.track_id && p->old_rows.state != p->new_rows.state && p->old_rows.birth_age != p->new_rows.birth_age &&
                p->old_rows.inactive_age != p->new_rows.inactive_age && p->old_rows.label != p->new_rows.label && p->old_rows.box != p->new_rows.box &&
                p->old_rows.trk_off != p->new_rows.trk_off, CNL_E_BAD_ARG, "%s: the new row arrays must not alias the old ones", name);
    CNL_REQUIRE((((uintptr_t)p->src_trk | (uintptr_t)p->src_det | (uintptr_t)p->flags | (uintptr_t)p->live) & 3) == 0 && ((uintptr_t)p->workspace & 7) == 0,
                CNL_E_BAD_ARG, "%s: src_trk, src_det, flags and live must be 4-byte aligned, the workspace 8-byte aligned", name);
    CNL_REQUIRE(p->workspace_bytes >= stage_bytes(p->S, p->max_tracks), CNL_E_BAD_ARG, "%s: workspace holds %ld bytes, S = %d, max_tracks = %d needs %ld", name,
                (long)p->workspace_bytes, p->S, p->max_tracks, stage_bytes(p->S, p->max_tracks));
    return CNL_OK;
}

}  // namespace cnl_lifecycle
using namespace cnl_lifecycle;

extern "C" int64_t cnl_track_lifecycle_workspace_bytes(int32_t S, int32_t max_tracks) {
    if (S <= 0 || max_tracks <= 0) return 0;
    return stage_bytes(S, max_tracks);
}

extern "C" int cnl_track_shift_f64(float* trk_box, double* box, double* kx, const int32_t* trk_off, const int32_t* live, const float* shift,
                                   int32_t* status, int32_t S, int32_t S_live, int32_t max_tracks, int32_t step, void* stream) {
    const char* name = "cnl_track_shift_f64";
    CNL_REQUIRE(trk_box && box && trk_off && live && shift && status, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(S > 0 && S <= MAX_STREAMS && S_live > 0 && S_live <= S && max_tracks > 0 && max_tracks <= MAX_TRACKS, CNL_E_BAD_ARG,
                "%s: bad S / S_live / max_tracks (%d / %d / %d)", name, S, S_live, max_tracks);
    CNL_REQUIRE((((uintptr_t)trk_box | (uintptr_t)trk_off | (uintptr_t)live | (uintptr_t)shift | (uintptr_t)status) & 3) == 0 &&
                (((uintptr_t)box | (uintptr_t)kx) & 7) == 0, CNL_E_BAD_ARG,
                "%s: trk_box, trk_off, live, shift and status must be 4-byte aligned, box and kx 8-byte aligned", name);
    hipLaunchKernelGGL(shift_kernel, dim3((unsigned)S_live), dim3(64), 0, (hipStream_t)stream, trk_box, box, kx, trk_off, live, shift, status, S, max_tracks,
                       step);
    return cnl::check_launch("track shift_kernel");
}

extern "C" int cnl_track_lifecycle_i32(const cnl_track_lifecycle* p, void* stream) {
    const char* name = "cnl_track_lifecycle_i32";
    if (int rc = check_args(name, p)) return rc;
    CNL_REQUIRE(p->slot_of && p->record && p->next_track_id && p->status, CNL_E_BAD_ARG, "%s: null pointer (slot_of / record / next_track_id / status)", name);
    CNL_REQUIRE(((uintptr_t)p->record & 7) == 0 && (p->record_stride & 7) == 0 && ((uintptr_t)p->next_track_id & 7) == 0 &&
                (((uintptr_t)p->slot_of | (uintptr_t)p->status) & 3) == 0, CNL_E_BAD_ARG,
                "%s: record, record_stride and next_track_id must be 8-byte aligned, slot_of and status 4-byte aligned", name);
    CNL_REQUIRE(p->record_stride >= (p->low_record ? 96 : 64), CNL_E_BAD_ARG, "%s: record_stride %ld below the record's header", name, (long)p->record_stride);
    CNL_REQUIRE(p->label_kind >= 0 && p->label_kind <= 3 && (p->label_kind == 0 || p->det_label), CNL_E_BAD_ARG,
                "%s: label_kind must be 0 (none), 1 (int64), 2 (int32), 3 (float32) with det_label set", name);
    CNL_REQUIRE(p->min_birth_age >= 0 && p->max_inactive_age >= 0, CNL_E_BAD_ARG, "%s: negative min_birth_age / max_inactive_age", name);
    hipLaunchKernelGGL(lifecycle_kernel, dim3((unsigned)p->S), dim3(64), 0, (hipStream_t)stream, *p);
    if (int rc = cnl::check_launch("track lifecycle_kernel")) return rc;
    const long C = (long)p->S * p->max_tracks;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p);
    return cnl::check_launch("track pack_kernel");
}

extern "C" int cnl_track_lifecycle_emit_f64(const cnl_track_lifecycle* p, void* stream) {
    const char* name = "cnl_track_lifecycle_emit_f64";
    if (int rc = check_args(name, p)) return rc;
    CNL_REQUIRE(p->det_box && ((uintptr_t)p->det_box & 3) == 0 && ((uintptr_t)p->kalman_box & 7) == 0, CNL_E_BAD_ARG,
                "%s: det_box null or not 4-byte aligned, or kalman_box not 8-byte aligned", name);
    CNL_REQUIRE(p->S_live == 0 || (p->out_box && p->out_track_id && p->out_label && p->out_count), CNL_E_BAD_ARG, "%s: null pointer (outputs)", name);
    CNL_REQUIRE((((uintptr_t)p->out_box | (uintptr_t)p->out_track_id | (uintptr_t)p->out_label) & 7) == 0 && ((uintptr_t)p->out_count & 3) == 0, CNL_E_BAD_ARG,
                "%s: out_box, out_track_id and out_label must be 8-byte aligned, out_count 4-byte aligned", name);
    const long C = (long)p->S * p->max_tracks;
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)(p->S_live + (C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *p);
    return cnl::check_launch("track emit_kernel");
}
