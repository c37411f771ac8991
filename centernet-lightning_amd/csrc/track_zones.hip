// track_zones.hip — zone occupancy, line crossings and dwell events from the output tensors of a TrackerBank(lifecycle="device") step
// (include/centernet_gfx950.h: cnl_track_zones_f64), ONE launch behind the bank's step.  The rule is the header's; tests/zones_ref.py restates
// it in numpy and is held equal to it bit for bit, so all geometry is float64 with one rounding per operation: no contraction (the pragma below
// and the Makefile's -ffp-contract=off).
//
//   zones_kernel   one workgroup of four waves per slot (and one per stream that takes no part, which copies its state to the other bank).
//                  The stream's geometry record, the ids of its previous list and a matched byte per entry live in LDS.
//                  Phase A, the output rows in chunks of 256, one row per thread: anchor, the first previous entry with the row's id (a linear
//                  walk of the LDS ids: every lane reads the same word), zones, lines, the row's new list entry at the rank of the present rows
//                  (ballot + popcount prefix), its events at the rank of the events (shuffle scan).  Phase B, the previous entries in chunks
//                  of 256: an unmatched entry ages, is carried behind the present rows at the rank of the kept entries, or expires with its
//                  exit events.  The step's counts are ballot popcounts added to LDS integers; every global word has one writer, no float
//                  atomics: the same bits on every run.  The old bank is only read, the new bank only written.
#pragma clang fp contract(off)
#include "cnl_common.h"

namespace cnl_zones {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_Z = 16, MAX_LN = 16, MAX_TRACKS = 4096, MAX_STREAMS = 65535, MAX_EVENTS = 65536;

struct ZoneRec {                        // 336 bytes
    int32_t n_vertices, dwell_alert, n_labels, reserved;
    int64_t labels[8];
    double v[16][2];
};
struct LineRec {                        // 104 bytes
    double ax, ay, bx, by;
    int32_t n_labels, reserved;
    int64_t labels[8];
};
static_assert(sizeof(ZoneRec) == 336 && sizeof(LineRec) == 104 && sizeof(cnl_track_zones) == 168, "record sizes of the header");

__host__ __device__ inline int64_t geometry_bytes(int Z, int Ln) { return 8 + 336 * (int64_t)Z + 104 * (int64_t)Ln; }
__host__ __device__ inline int64_t stream_bytes(int E, int Z, int Ln) { return 16 * (int64_t)Z + 16 * (int64_t)Ln + 8 + (int64_t)E * (32 + 4 * Z); }
__host__ inline int lds_bytes(int E, int Z, int Ln) { return (int)geometry_bytes(Z, Ln) + 8 * E + ((E + 7) & ~7); }

// one stream's state in one bank
struct StreamState {
    int64_t* zone_counts;       // [Z, 2]
    int64_t* line_counts;       // [Ln, 2]
    int32_t* n_entries;         // [2]: the count, a zero
    int64_t* id;                // [E]
    double* anchor;             // [E, 2]
    int32_t* inside;            // [E]
    int32_t* age;               // [E]
    int32_t* dwell;             // [E, Z]
};
__device__ __forceinline__ StreamState carve(char* base, int E, int Z, int Ln) {
    StreamState st;
    st.zone_counts = (int64_t*)base;
    st.line_counts = st.zone_counts + 2 * Z;
    st.n_entries = (int32_t*)(st.line_counts + 2 * Ln);
    st.id = (int64_t*)(st.n_entries + 2);
    st.anchor = (double*)(st.id + E);
    st.inside = (int32_t*)(st.anchor + 2 * (size_t)E);
    st.age = st.inside + E;
    st.dwell = st.age + E;
    return st;
}

// The exclusive prefix of v over the workgroup in thread order, and the total (two barriers; s_w: WAVES ints).
__device__ __forceinline__ int block_prefix(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        if (i < w) base += s_w[i];
        total += s_w[i];
    }
    __syncthreads();
    return base + inc - v;
}
// The same for a flag: ballot + popcount inside the wave.
__device__ __forceinline__ int block_rank(bool flag, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        if (i < w) base += s_w[i];
        total += s_w[i];
    }
    __syncthreads();
    return base + __popcll(m & ((1ull << lane) - 1ull));
}
// counter += the lanes of this wave whose flag is set (called by whole waves)
__device__ __forceinline__ void wave_count(bool flag, int* counter) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, __popcll(m));
}

__device__ __forceinline__ bool label_passes(int n_labels, const int64_t* labels, int64_t label) {
    if (n_labels <= 0) return true;
    bool ok = false;
    for (int j = 0; j < n_labels; ++j) ok |= labels[j] == label;
    return ok;
}

// even-odd rule without a division (the header's rule 2)
__device__ __forceinline__ bool in_polygon(const ZoneRec& zr, double px, double py) {
    bool in = false;
    const int nv = zr.n_vertices;
    for (int a = 0; a < nv; ++a) {
        const int b = a + 1 == nv ? 0 : a + 1;
        const double xi = zr.v[a][0], yi = zr.v[a][1], xj = zr.v[b][0], yj = zr.v[b][1];
        if ((yi > py) != (yj > py)) {
            const double t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi);
            if (yj > yi ? t > 0.0 : t < 0.0) in = !in;
        }
    }
    return in;
}

__device__ __forceinline__ double cross(double ux, double uy, double vx, double vy) { return ux * vy - uy * vx; }

// 0: no crossing, 3: forward, 4: backward (the header's rule 3)
__device__ __forceinline__ int line_crossing(const LineRec& lr, double p0x, double p0y, double p1x, double p1y) {
    const double bx = lr.bx - lr.ax, by = lr.by - lr.ay;
    const bool d0 = cross(bx, by, p0x - lr.ax, p0y - lr.ay) > 0.0, d1 = cross(bx, by, p1x - lr.ax, p1y - lr.ay) > 0.0;
    if (d0 == d1) return 0;
    const double sx = p1x - p0x, sy = p1y - p0y;
    const bool e0 = cross(sx, sy, lr.ax - p0x, lr.ay - p0y) > 0.0, e1 = cross(sx, sy, lr.bx - p0x, lr.by - p0y) > 0.0;
    if (e0 == e1) return 0;
    return d1 ? 3 : 4;
}

__device__ __forceinline__ void emit(const cnl_track_zones& a, int slot, int k, int64_t id, int kind, int index, int64_t value) {
    if (k < a.max_events) {
        int64_t* ev = a.events + ((size_t)slot * a.max_events + k) * 4;
        ev[0] = id; ev[1] = kind; ev[2] = index; ev[3] = value;
    }
}

__global__ __launch_bounds__(THREADS) void zones_kernel(const cnl_track_zones a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ int s_w[WAVES];
    __shared__ int s_enter[MAX_Z], s_exit[MAX_Z], s_occ[MAX_Z], s_fwd[MAX_LN], s_bwd[MAX_LN];
    __shared__ int s_status;
    const int tid = threadIdx.x, slot = blockIdx.x;
    const int S = a.S, M = a.M, Z = a.Z, Ln = a.Ln, E = 2 * a.max_tracks;
    const int s = a.live[slot];
    if (s < 0 || s >= S) return;                                      // uniform
    const int64_t sb = stream_bytes(E, Z, Ln);
    char* const state = (char*)a.state;
    char* const old_base = state + ((int64_t)a.bank * S + s) * sb;
    char* const new_base = state + ((int64_t)(1 - a.bank) * S + s) * sb;
    if (slot >= a.L) {                                                // a stream that takes no part: carried untouched into the other bank
        const int64_t* src = (const int64_t*)old_base;
        int64_t* dst = (int64_t*)new_base;
        const int64_t words = sb >> 3;
        for (int64_t i = tid; i < words; i += THREADS) dst[i] = src[i];
        return;
    }
    const StreamState old = carve(old_base, E, Z, Ln), nw = carve(new_base, E, Z, Ln);
    const int gb = (int)geometry_bytes(Z, Ln);
    const ZoneRec* const zones = (const ZoneRec*)(lds + 8);
    const LineRec* const lines = (const LineRec*)(lds + 8 + 336 * Z);
    int64_t* const s_id = (int64_t*)(lds + gb);
    unsigned char* const s_hit = (unsigned char*)(lds + gb + 8 * (size_t)E);
    const int n_prev = min(max(old.n_entries[0], 0), E);
    {
        const int64_t* g = (const int64_t*)((const char*)a.geometry + (int64_t)s * gb);
        for (int i = tid; i < gb / 8; i += THREADS) ((int64_t*)lds)[i] = g[i];
        for (int i = tid; i < n_prev; i += THREADS) { s_id[i] = old.id[i]; s_hit[i] = 0; }
        if (tid < MAX_Z) { s_enter[tid] = 0; s_exit[tid] = 0; s_occ[tid] = 0; s_fwd[tid] = 0; s_bwd[tid] = 0; }
        if (tid == 0) s_status = 0;
    }
    __syncthreads();
    const int n_lines = min(max(((const int32_t*)lds)[1], 0), Ln);
    const int n = min(max(a.count[slot], 0), M);
    int n_present = 0, n_events = 0, status = 0;                      // n_present, n_events: uniform running totals

    // Phase A: the output rows
    for (int base = 0; base < M; base += THREADS) {
        const int r = base + tid;
        const size_t row = (size_t)slot * M + r;
        double px = 0.0, py = 0.0;
        bool present = false;
        if (r < n) {
            double x1, y1, x2, y2;
            if (a.boxes_f64) {
                const double* b = (const double*)a.boxes + row * 4;
                x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3];
            } else {
                const float* b = (const float*)a.boxes + row * 4;
                x1 = (double)b[0]; y1 = (double)b[1]; x2 = (double)b[2]; y2 = (double)b[3];
            }
            px = (x1 + x2) * 0.5;
            py = a.anchor ? (y1 + y2) * 0.5 : y2;
            present = isfinite(px) && isfinite(py);
            if (!present) status |= 1;
        }
        int total;
        const int pos = n_present + block_rank(present, s_w, total);
        n_present += total;

        int64_t id = 0, label = 0;
        int e = -1, prev_inside = 0;
        double p0x = 0.0, p0y = 0.0;
        if (present) {
            id = a.track_ids[row];
            label = a.labels[row];
            for (int j = 0; j < n_prev; ++j)
                if (s_id[j] == id) { e = j; break; }
            if (e >= 0) {
                s_hit[e] = 1;
                prev_inside = old.inside[e];
                p0x = old.anchor[2 * (size_t)e];
                p0y = old.anchor[2 * (size_t)e + 1];
            }
        }
        int inside = 0, enter = 0, leave = 0, alert = 0, fwd = 0, bwd = 0;
        for (int z = 0; z < Z; ++z) {                                 // uniform trip counts: whole waves reach the ballots
            const ZoneRec& zr = zones[z];
            const bool in = present && label_passes(zr.n_labels, zr.labels, label) && in_polygon(zr, px, py);
            const bool was = (prev_inside >> z) & 1;
            int dwell = 0;
            if (in) dwell = was ? old.dwell[(size_t)e * Z + z] + 1 : 1;
            if (r < M) a.dwell[row * Z + z] = dwell;
            if (present) nw.dwell[(size_t)pos * Z + z] = dwell;
            const bool al = in && zr.dwell_alert > 0 && dwell == zr.dwell_alert;
            inside |= (int)in << z;
            enter |= (int)(in && !was) << z;
            leave |= (int)(!in && was) << z;
            alert |= (int)al << z;
            wave_count(in, &s_occ[z]);
            wave_count(in && !was, &s_enter[z]);
            wave_count(!in && was, &s_exit[z]);
        }
        for (int l = 0; l < n_lines; ++l) {
            const LineRec& lr = lines[l];
            int kind = 0;
            if (e >= 0 && label_passes(lr.n_labels, lr.labels, label)) kind = line_crossing(lr, p0x, p0y, px, py);
            fwd |= (int)(kind == 3) << l;
            bwd |= (int)(kind == 4) << l;
            wave_count(kind == 3, &s_fwd[l]);
            wave_count(kind == 4, &s_bwd[l]);
        }
        if (r < M) a.inside[row] = inside;
        if (present) {
            nw.id[pos] = id;
            nw.anchor[2 * (size_t)pos] = px;
            nw.anchor[2 * (size_t)pos + 1] = py;
            nw.inside[pos] = inside;
            nw.age[pos] = 0;
        }
        const int mine = __popc(enter) + __popc(leave) + __popc(alert) + __popc(fwd) + __popc(bwd);
        int k = n_events + block_prefix(mine, s_w, total);
        n_events += total;
        if (mine) {
            for (int z = 0; z < Z; ++z) {
                if ((leave >> z) & 1) emit(a, slot, k++, id, 2, z, old.dwell[(size_t)e * Z + z]);
                if ((enter >> z) & 1) emit(a, slot, k++, id, 1, z, e < 0 ? 1 : 0);
                if ((alert >> z) & 1) emit(a, slot, k++, id, 5, z, zones[z].dwell_alert);
            }
            for (int l = 0; l < n_lines; ++l) {
                if ((fwd >> l) & 1) emit(a, slot, k++, id, 3, l, 0);
                if ((bwd >> l) & 1) emit(a, slot, k++, id, 4, l, 0);
            }
        }
    }
    __syncthreads();                                                  // every s_hit is written

    // Phase B: the previous entries no present row took
    int n_kept = 0;
    for (int base = 0; base < n_prev; base += THREADS) {
        const int e = base + tid;
        const bool absent = e < n_prev && !s_hit[e];
        const int age = absent ? old.age[e] + 1 : 0;
        const bool expired = absent && age > a.max_absent, kept = absent && !expired;
        const int was = absent ? old.inside[e] : 0;
        int total;
        const int pos = n_present + n_kept + block_rank(kept, s_w, total);
        n_kept += total;
        if (kept) {
            if (pos < E) {
                nw.id[pos] = s_id[e];
                nw.anchor[2 * (size_t)pos] = old.anchor[2 * (size_t)e];
                nw.anchor[2 * (size_t)pos + 1] = old.anchor[2 * (size_t)e + 1];
                nw.inside[pos] = was;
                nw.age[pos] = age;
                for (int z = 0; z < Z; ++z) nw.dwell[(size_t)pos * Z + z] = old.dwell[(size_t)e * Z + z];
            } else {
                status |= 2;
            }
        }
        const int mine = expired ? __popc(was) : 0;
        int k = n_events + block_prefix(mine, s_w, total);
        n_events += total;
        for (int z = 0; z < Z; ++z) {
            const bool out = expired && ((was >> z) & 1);
            if (out) emit(a, slot, k++, s_id[e], 2, z, old.dwell[(size_t)e * Z + z]);
            wave_count(out, &s_exit[z]);
        }
    }
    if (n_events > a.max_events) status |= 4;
    if (status) atomicOr(&s_status, status);
    __syncthreads();

    if (tid < Z) {
        const int64_t in = old.zone_counts[2 * tid] + s_enter[tid], out = old.zone_counts[2 * tid + 1] + s_exit[tid];
        nw.zone_counts[2 * tid] = in;
        nw.zone_counts[2 * tid + 1] = out;
        a.zone_counts[((size_t)slot * Z + tid) * 2] = in;
        a.zone_counts[((size_t)slot * Z + tid) * 2 + 1] = out;
        a.occupancy[(size_t)slot * Z + tid] = s_occ[tid];
    }
    if (tid < Ln) {
        const int64_t f = old.line_counts[2 * tid] + s_fwd[tid], b = old.line_counts[2 * tid + 1] + s_bwd[tid];
        nw.line_counts[2 * tid] = f;
        nw.line_counts[2 * tid + 1] = b;
        a.line_counts[((size_t)slot * Ln + tid) * 2] = f;
        a.line_counts[((size_t)slot * Ln + tid) * 2 + 1] = b;
    }
    if (tid == 0) {
        nw.n_entries[0] = min(n_present + n_kept, E);
        nw.n_entries[1] = 0;
        a.event_count[slot] = n_events;
        const int bits = s_status;
        if (bits) {                                                   // sticky: this workgroup is the word's only writer
            const int w = a.status[2 * s];
            if (w == 0) a.status[2 * s + 1] = a.step;
            a.status[2 * s] = w | bits;
        }
    }
    int64_t* const ev = a.events + (size_t)slot * a.max_events * 4;  // zero rows behind the live ones
    for (int i = min(n_events, a.max_events) * 4 + tid; i < a.max_events * 4; i += THREADS) ev[i] = 0;
}

static cnl::DeviceOnce g_once;

}  // namespace cnl_zones
using namespace cnl_zones;

extern "C" int64_t cnl_track_zones_state_bytes(int32_t S, int32_t max_tracks, int32_t Z, int32_t Ln) {
    if (S <= 0 || S > MAX_STREAMS || max_tracks <= 0 || max_tracks > MAX_TRACKS || Z < 0 || Z > MAX_Z || Ln < 0 || Ln > MAX_LN) return 0;
    return 2 * (int64_t)S * stream_bytes(2 * max_tracks, Z, Ln);
}

extern "C" int cnl_track_zones_f64(const cnl_track_zones* p, void* stream) {
    const char* name = "cnl_track_zones_f64";
    CNL_REQUIRE(p, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(p->S >= 1 && p->S <= MAX_STREAMS && p->L >= 1 && p->L <= p->S, CNL_E_BAD_ARG,
                "%s: S = %d, L = %d: expected S in 1 .. %d and 1 <= L <= S (a slot outside the S streams)", name, p->S, p->L, MAX_STREAMS);
    CNL_REQUIRE(p->max_tracks >= 1 && p->max_tracks <= MAX_TRACKS, CNL_E_BAD_ARG, "%s: max_tracks = %d, expected 1 .. %d", name, p->max_tracks, MAX_TRACKS);
    CNL_REQUIRE(p->M >= 1 && p->M <= p->max_tracks, CNL_E_BAD_ARG, "%s: M = %d rows, expected 1 .. max_tracks = %d", name, p->M, p->max_tracks);
    CNL_REQUIRE(p->Z >= 0 && p->Z <= MAX_Z && p->Ln >= 0 && p->Ln <= MAX_LN, CNL_E_BAD_ARG, "%s: Z = %d, Ln = %d: expected 0 .. 16 each", name, p->Z, p->Ln);
    CNL_REQUIRE(p->max_events >= 1 && p->max_events <= MAX_EVENTS && p->max_absent >= 0, CNL_E_BAD_ARG,
                "%s: max_events = %d, max_absent = %d: expected 1 .. %d and >= 0", name, p->max_events, p->max_absent, MAX_EVENTS);
    CNL_REQUIRE((p->anchor == 0 || p->anchor == 1) && (p->boxes_f64 == 0 || p->boxes_f64 == 1) && (p->bank == 0 || p->bank == 1), CNL_E_BAD_ARG,
                "%s: anchor = %d, boxes_f64 = %d, bank = %d: expected 0 or 1 each", name, p->anchor, p->boxes_f64, p->bank);
    CNL_REQUIRE(p->boxes && p->track_ids && p->labels && p->count && p->live && p->geometry && p->state && p->status && p->inside && p->events &&
                p->event_count, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE((p->Z == 0 || (p->dwell && p->occupancy && p->zone_counts)) && (p->Ln == 0 || p->line_counts), CNL_E_BAD_ARG,
                "%s: null pointer (dwell / occupancy / zone_counts with Z > 0, line_counts with Ln > 0)", name);
    CNL_REQUIRE((((uintptr_t)p->track_ids | (uintptr_t)p->labels | (uintptr_t)p->geometry | (uintptr_t)p->state | (uintptr_t)p->zone_counts |
                  (uintptr_t)p->line_counts | (uintptr_t)p->events) & 7) == 0 && ((uintptr_t)p->boxes & (p->boxes_f64 ? 7 : 3)) == 0 &&
                (((uintptr_t)p->count | (uintptr_t)p->live | (uintptr_t)p->status | (uintptr_t)p->inside | (uintptr_t)p->dwell |
                  (uintptr_t)p->occupancy | (uintptr_t)p->event_count) & 3) == 0, CNL_E_BAD_ARG,
                "%s: int64 / float64 arrays, geometry and state must be 8-byte aligned, the others 4-byte aligned", name);
    const int lds = lds_bytes(2 * p->max_tracks, p->Z, p->Ln);
    if (int rc = cnl::kernel_setup(g_once, (const void*)zones_kernel, lds_bytes(2 * MAX_TRACKS, MAX_Z, MAX_LN))) return rc;
    hipLaunchKernelGGL(zones_kernel, dim3((unsigned)p->S), dim3(THREADS), (size_t)lds, (hipStream_t)stream, *p);
    return cnl::check_launch("track zones_kernel");
}
