// augment_common.h — the ONE copy of what augment.hip (window -> rectangle placements, the separable cv2 rule) and augment_warp.hip (affine
// placements, the Q20 inverse-map rule) both do AFTER a pixel or a box has been carried through its placement's geometry:
//   rect_ok / check_plan   the bounds of a destination rectangle (device) and of a plan's host-visible arguments (host)
//   colour_step            the Q12 colour matrix of one pixel, with the guard that keeps the compiler from packing two channels over stale bits
//   find_holes / punch     the holes that touch a tile, by one ballot of the first wave, and their fill over a thread's 4-pixel group
//   BoxOut / boxes_kernel  the float64 box rule from `full` on (clip, keep conditions, output), the stable ballot compaction with its zeroed tail, and
//                          the box kernel itself, a template over the placement's geometry
#pragma once
#include "letterbox_sampling.h"

#pragma clang fp contract(off)   // the box rule rounds every operation on its own

namespace cnl_augment {

using namespace cnl_letterbox;

constexpr int MAX_PLACE = 4, MAX_HOLES = 16, BOX_THREADS = 256;

// a destination rectangle the pixel kernels paint: aligned to the 4-pixel groups, not empty, inside the canvas; no sum can overflow
__device__ __forceinline__ bool rect_ok(int dx0, int dy0, int dw, int dh, int width, int height) {
    return dw >= 4 && dh >= 1 && dx0 >= 0 && dy0 >= 0 && ((dx0 | dw) & 3) == 0 && dw <= width && dh <= height && dx0 <= width - dw && dy0 <= height - dh;
}

// (R, G, B) at bits 0, 8, 16 of px through the Q12 matrix m (m[3c + k] weighs source channel k in channel c, m[9 + c] is channel c's offset):
// |m| <= 32767 and |offset| <= 2^21 (the entries' contract): 3 * 255 * 32767 + 2^21 + 2^11 < 2^31
__device__ __forceinline__ unsigned colour_step(const int (&m)[12], unsigned px) {
    const int R = (int)(px & 255u), G = (int)((px >> 8) & 255u), B = (int)((px >> 16) & 255u);
    unsigned v = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int t = (m[3 * c] * R + m[3 * c + 1] * G + m[3 * c + 2] * B + m[9 + c] + 2048) >> 12;
        // the shifted value is made opaque before the clamp: left to itself the compiler fuses shift, clamp and the packing of two
        // channels into one v_ashr_pk_u8_i32 and ORs the third channel over the result's upper half, which that instruction does
        // not clear on gfx950 (seen as stray bits of m * G in the blue byte); shift, v_med3 and the shifts-and-ors cost the same
        asm volatile("" : "+v"(t));
        v |= (unsigned)min(max(t, 0), 255) << (8 * c);
    }
    return v;
}

// The first wave (tid < 64, all of its lanes call): the live hole slots of canvas n clipped to the canvas go to hole[], and hole_mask gets
// bit k set where hole k touches the tile [x_begin, x_end) x [row_begin, row_end).  The caller's next barrier publishes both.
__device__ __forceinline__ void find_holes(const int4* __restrict__ holes, int n, int tid, int width, int height, int x_begin, int x_end, int row_begin,
                                           int row_end, int4 (&hole)[MAX_HOLES], unsigned& hole_mask) {
    bool touches = false;
    if (holes && tid < MAX_HOLES) {
        const int4 q = holes[(size_t)n * MAX_HOLES + tid];     // (x0, y0, w, h); w <= 0 or h <= 0: a dead slot
        if (q.z > 0 && q.w > 0) {
            const long long xe = (long long)q.x + q.z, ye = (long long)q.y + q.w;
            const int4 c = make_int4(max(q.x, 0), max(q.y, 0), (int)min(xe, (long long)width), (int)min(ye, (long long)height));
            if (xe > 0 && ye > 0) {
                hole[tid] = c;
                touches = c.x < x_end && c.z > x_begin && c.y < row_end && c.w > row_begin;
            }
        }
    }
    const unsigned long long mask = __ballot(touches);
    if (tid == 0) hole_mask = (unsigned)mask;
}

// the group of four pixels at (y, x .. x + 3): hole_fill where a hole of the mask `touching` covers a pixel
__device__ __forceinline__ void punch(unsigned touching, const int4 (&hole)[MAX_HOLES], int y, int x, unsigned hole_fill, unsigned (&px)[4]) {
    for (unsigned left = touching; left; left &= left - 1) {
        const int4 h = hole[__builtin_ctz(left)];
        if (y >= h.y && y < h.w) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (x + p >= h.x && x + p < h.z) px[p] = hole_fill;
        }
    }
}

// One canvas's kept boxes: boxes_kernel (one workgroup of BOX_THREADS per canvas) maps a chunk of BOX_THREADS boxes through a placement, calls
// clip() on each and put() once per chunk with every thread, and finish() at the end.
struct BoxOut {
    double* ob;
    long long *ol, *oi;
    int Gout, base;                              // kept so far: uniform

    __device__ __forceinline__ BoxOut(double* out_boxes, long long* out_labels, long long* out_ids, int n, int Gout)
        : ob(out_boxes + (size_t)n * Gout * 4), ol(out_labels + (size_t)n * Gout), oi(out_ids ? out_ids + (size_t)n * Gout : nullptr), Gout(Gout), base(0) {}

    // The rule from `full` on: the box's extent [u1, u2] x [v1, v2] in rectangle coordinates with full = (u2 - u1) * (v2 - v1), `finite` saying
    // that the box, everything it was mapped to and full are finite -> kept or not, and (x, y, w, h) in canvas pixels.
    static __device__ __forceinline__ bool clip(double u1, double u2, double v1, double v2, double full, bool finite, int dx0, int dy0, double dw, double dh,
                                                long long label, double min_area, double min_visibility, double (&b)[4]) {
        b[0] = b[1] = b[2] = b[3] = 0;
        if (!finite) return false;
        const double cu1 = fmin(fmax(u1, 0.0), dw), cu2 = fmin(fmax(u2, 0.0), dw);
        const double cv1 = fmin(fmax(v1, 0.0), dh), cv2 = fmin(fmax(v2, 0.0), dh);
        b[2] = cu2 - cu1;
        b[3] = cv2 - cv1;
        const double area = b[2] * b[3];
        b[0] = (double)dx0 + cu1;
        b[1] = (double)dy0 + cv1;
        return b[2] > 0.0 && b[3] > 0.0 && area >= min_area && area >= min_visibility * full && label >= 0;
    }

    // stable compaction of one chunk by ballots and prefix counts (no atomics): wave_kept is BOX_THREADS / 64 ints of LDS
    __device__ __forceinline__ void put(bool keep, const double (&b)[4], long long label, long long id, int* wave_kept) {
        const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(kept);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < BOX_THREADS / 64; ++k) {
            const int c = wave_kept[k];
            before += k < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int pos = base + before + __popcll(kept & ((1ull << lane) - 1ull));
            if (pos < Gout) {
                ob[(size_t)pos * 4] = b[0];
                ob[(size_t)pos * 4 + 1] = b[1];
                ob[(size_t)pos * 4 + 2] = b[2];
                ob[(size_t)pos * 4 + 3] = b[3];
                ol[pos] = label;
                if (oi) oi[pos] = id;
            }
        }
        base += total;
        __syncthreads();                         // wave_kept is rewritten by the next chunk
    }

    // slots beyond the count are exactly zero
    __device__ __forceinline__ void finish(int* out_count, int n) {
        base = min(base, Gout);
        for (int j = base + (int)threadIdx.x; j < Gout; j += BOX_THREADS) {
            ob[(size_t)j * 4] = ob[(size_t)j * 4 + 1] = ob[(size_t)j * 4 + 2] = ob[(size_t)j * 4 + 3] = 0.0;
            ol[j] = 0;
            if (oi) oi[j] = 0;
        }
        if (threadIdx.x == 0) out_count[n] = base;
    }
};

// The box kernel of both rules.  Map is a placement's geometry: Map::Record the plan's record type, Map::live(q, F) whether a record carries
// boxes, Map(q).extent(x, y, w, h, u1, u2, v1, v2) the box's extent in rectangle coordinates (-> everything it was mapped to is finite).
// One workgroup per canvas; placements in slot order, boxes in source order, in chunks of BOX_THREADS.
template <class Map>
__global__ __launch_bounds__(BOX_THREADS) void boxes_kernel(const typename Map::Record* __restrict__ places, const int* __restrict__ n_place, int F, int max_place,
                                                            const double* __restrict__ boxes, const long long* __restrict__ labels,
                                                            const long long* __restrict__ ids, const int* __restrict__ count, int Gmax,
                                                            double* __restrict__ out_boxes, long long* __restrict__ out_labels, long long* __restrict__ out_ids,
                                                            int* __restrict__ out_count, int Gout, double min_area, double min_visibility) {
    __shared__ int wave_kept[BOX_THREADS / 64];
    const int n = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int np = min(max(n_place[n], 0), max_place);
    BoxOut out(out_boxes, out_labels, out_ids, n, Gout);
    for (int p = 0; p < np; ++p) {
        const typename Map::Record q = places[(size_t)n * MAX_PLACE + p];        // uniform address: scalar loads
        if (!Map::live(q, F)) continue;
        const Map map(q);
        const int cnt = min(max(count[q.frame], 0), Gmax);
        const double dw = (double)q.dw, dh = (double)q.dh;
        for (int j0 = 0; j0 < cnt; j0 += BOX_THREADS) {
            const int j = j0 + tid;
            bool keep = false;
            double b[4] = {0, 0, 0, 0};
            long long label = 0, id = 0;
            if (j < cnt) {
                const size_t s = (size_t)q.frame * Gmax + j;
                const double x = boxes[s * 4], y = boxes[s * 4 + 1], w = boxes[s * 4 + 2], h = boxes[s * 4 + 3];
                label = labels[s];
                if (ids) id = ids[s];
                double u1, u2, v1, v2;
                const bool mapped = map.extent(x, y, w, h, u1, u2, v1, v2);
                const double full = (u2 - u1) * (v2 - v1);
                const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(w) && __builtin_isfinite(h) && mapped &&
                                    __builtin_isfinite(full);
                keep = BoxOut::clip(u1, u2, v1, v2, full, finite, q.dx0, q.dy0, dw, dh, label, min_area, min_visibility, b);
            }
            out.put(keep, b, label, id, wave_kept);
        }
    }
    out.finish(out_count, n);
}

// ----------------------------------------------------------------------------- host: what both pairs of entry points check alike
static int check_plan(const char* entry, const void* places, const int32_t* n_place, int N, int F, int max_place) {
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "%s: N = %d outside 0..65535", entry, N);
    CNL_REQUIRE(F >= 0 && F <= 65535, CNL_E_BAD_ARG, "%s: F = %d outside 0..65535", entry, F);
    CNL_REQUIRE(max_place >= 1 && max_place <= MAX_PLACE, CNL_E_BAD_ARG, "%s: max_place = %d outside 1..%d", entry, max_place, MAX_PLACE);
    if (N == 0) return CNL_OK;                   // an empty batch is a no-op: its pointers are not looked at
    CNL_REQUIRE(places && n_place, CNL_E_BAD_ARG, "%s: null plan pointer", entry);
    CNL_REQUIRE(((uintptr_t)places & 7) == 0 && ((uintptr_t)n_place & 3) == 0, CNL_E_BAD_ARG, "%s: places must be 8-byte and n_place 4-byte aligned", entry);
    return CNL_OK;
}

static int check_canvas(const char* entry, const void* frames, int F, const void* holes, const void* out, int N, int height, int width) {
    CNL_REQUIRE(height >= 1 && height <= 32768 && width >= 4 && width <= 32768 && width % 4 == 0, CNL_E_BAD_ARG,
                "%s: canvas %d x %d needs a height in 1..32768 and a width in 4..32768 that is a multiple of 4", entry, height, width);
    CNL_REQUIRE((long)height * width * 3 <= 0x7fffffffL, CNL_E_BAD_ARG, "%s: one canvas exceeds 2 GiB", entry);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(out && (frames || F == 0), CNL_E_BAD_ARG, "%s: null pointer", entry);
    CNL_REQUIRE(((uintptr_t)frames & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)holes & 15) == 0, CNL_E_BAD_ARG,
                "%s: frames must be 8-byte, out 4-byte and holes 16-byte aligned", entry);
    return CNL_OK;
}

static int check_boxes(const char* entry, int N, int F, int max_place, const double* boxes, const int64_t* labels, const int64_t* ids, const int32_t* count,
                       int Gmax, double* out_boxes, int64_t* out_labels, int64_t* out_ids, int32_t* out_count, int Gout, double min_area,
                       double min_visibility) {
    CNL_REQUIRE(Gmax >= 1 && Gmax <= 65535, CNL_E_BAD_ARG, "%s: Gmax = %d outside 1..65535", entry, Gmax);
    CNL_REQUIRE(Gout >= max_place * Gmax, CNL_E_BAD_ARG, "%s: Gout = %d is smaller than max_place * Gmax = %d", entry, Gout, max_place * Gmax);
    CNL_REQUIRE(min_area == min_area && min_visibility == min_visibility, CNL_E_BAD_ARG, "%s: min_area or min_visibility is NaN", entry);
    CNL_REQUIRE((ids == nullptr) == (out_ids == nullptr), CNL_E_BAD_ARG, "%s: ids and out_ids are given together", entry);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(out_boxes && out_labels && out_count && (F == 0 || (boxes && labels && count)), CNL_E_BAD_ARG, "%s: null pointer", entry);
    CNL_REQUIRE(((uintptr_t)boxes & 7) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)ids & 7) == 0 && ((uintptr_t)count & 3) == 0 &&
                    ((uintptr_t)out_boxes & 7) == 0 && ((uintptr_t)out_labels & 7) == 0 && ((uintptr_t)out_ids & 7) == 0 && ((uintptr_t)out_count & 3) == 0,
                CNL_E_BAD_ARG, "%s: boxes, labels and ids must be 8-byte, counts 4-byte aligned", entry);
    return CNL_OK;
}

// the canvas tiling both pixel kernels launch on: equal column tiles of at most LB_TILE_GROUPS groups, blocks of LB_ROWS rows
struct CanvasGrid {
    int tiles_x, groups_per_tile, row_blocks;
    CanvasGrid(int height, int width) {
        const int groups = width / 4;
        tiles_x = (groups + LB_TILE_GROUPS - 1) / LB_TILE_GROUPS;
        groups_per_tile = (groups + tiles_x - 1) / tiles_x;                    // equal tiles, as letterbox_kernel's launch
        row_blocks = (height + LB_ROWS - 1) / LB_ROWS;
    }
};

}  // namespace cnl_augment
