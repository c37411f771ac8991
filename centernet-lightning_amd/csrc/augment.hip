// augment.hip — the training augmentation of a batch on the device: the reference's albumentations Compose (HorizontalFlip,
// RandomResizedCrop, ColorJitter, Cutout; datasets/builder.py::parse_transforms, one image at a time in DataLoader workers) and the batch-level
// Mosaic that datasets/transforms.py declares and never wrote, as a deterministic function of a PLAN the host drew.
//
//   augment_kernel        up to four placements per canvas (a window of a source frame -> a rectangle of the canvas), each mirrored or not and
//                         with its own Q12 colour matrix, then the holes: [N, height, width, 3] u8 in ONE launch that writes every canvas byte
//                         exactly once (no memset, no atomics).  The sampling rule is letterbox_kernel's, from the one copy in
//                         letterbox_sampling.h: a placement without flip, colour or holes is bit for bit cnl_letterbox_bilinear_u8.
//   augment_boxes_kernel  the targets through the same plan in float64, one rounding per operation (fp contract is off), filtered by
//                         albumentations' BboxParams rule and compacted stably with ballots and prefix counts: no atomics, the same bits on
//                         every run.
//
// Decomposition of augment_kernel: letterbox_kernel's.  grid.y = canvas, grid.x = (block of LB_ROWS canvas rows) x (column tile of <= 1024
// columns): the CANVAS is tiled, so a 1080p source and a 7 x 5 source cost the same.  The first four threads turn the canvas's placement records
// into descriptors in LDS (the window as a source, the rectangle, the matrix; a degenerate record is not live and paints nothing).  For every live
// placement the tile touches — at most four — the workgroup builds that placement's column table (for the tile's columns inside its rectangle;
// a mirrored placement keeps the coefficients of column dw - 1 - dx at column dx) and its row table, once, in LDS.  A thread owns 4 neighbouring
// pixels = three whole 32-bit words; dx0 % 4 == 0 and dw % 4 == 0 mean a group never straddles two placements, so a group has ONE placement or
// none and its eight tap loads are PackedSource<3>'s unaligned 8-byte loads.  The holes that touch the tile are found by one ballot of the first
// wave; a thread loops over that mask only.
#include "letterbox_sampling.h"

#pragma clang fp contract(off)   // the sampling rule and the box rule round every operation on its own

namespace cnl_augment {

using namespace cnl_letterbox;

constexpr int MAX_PLACE = 4, MAX_HOLES = 16, BOX_THREADS = 256;
typedef PackedSource<3> Source;
static_assert(sizeof(cnl_augment_placement) == 96, "cnl_augment_placement is 96 bytes");
static_assert(sizeof(cnl_letterbox_frame) == 40, "cnl_letterbox_frame is 40 bytes");

// one placement as the workgroup uses it
struct Placement {
    const void* src;                 // the window's first pixel
    int row_stride, w, h;            // the window as a packed source
    int live;
    int x0, y0, x1, y1;              // the rectangle in canvas pixels, [x0, x1) x [y0, y1)
    int dw, dh, flip, pad;
    int m[12];                       // Q12: m[3c + k] = weight of source channel k in channel c, m[9 + c] = offset of channel c
};

__global__ __launch_bounds__(LB_THREADS) void augment_kernel(const cnl_letterbox_frame* __restrict__ frames, int F,
                                                             const cnl_augment_placement* __restrict__ places, const int* __restrict__ n_place,
                                                             const int4* __restrict__ holes, unsigned char* __restrict__ out, int height, int width,
                                                             int max_place, unsigned fill, unsigned hole_fill, int tiles_x, int groups_per_tile) {
    // col[p]: .x = byte offset of the left tap in a window row, .y = a0 | a1 << 16; written (and read) inside placement p's rectangle only
    __shared__ __attribute__((aligned(16))) int2 col[MAX_PLACE][LB_TILE_GROUPS * 4];
    __shared__ int4 row[MAX_PLACE][LB_ROWS];     // .x = y0, .y = y1, .z = b0, .w = b1
    __shared__ Placement place[MAX_PLACE];
    __shared__ int4 hole[MAX_HOLES];             // .x .y = first column / row, .z .w = one past the last, clipped to the canvas
    __shared__ unsigned hole_mask;               // bit k: hole k touches this tile

    const int n = (int)blockIdx.y;
    const int tile = (int)(blockIdx.x % (unsigned)tiles_x), rblk = (int)(blockIdx.x / (unsigned)tiles_x);
    const int groups = width >> 2;
    const int g_begin = tile * groups_per_tile, g_end = min(groups, g_begin + groups_per_tile);
    const int n_groups = g_end - g_begin;
    const int x_begin = g_begin * 4, x_end = g_end * 4;
    const int row_begin = rblk * LB_ROWS, n_rows = min(LB_ROWS, height - row_begin), row_end = row_begin + n_rows;
    const int tid = (int)threadIdx.x;

    if (tid < MAX_PLACE) {
        Placement e = {};
        const int np = min(max(n_place[n], 0), max_place);
        if (tid < np) {
            const cnl_augment_placement q = places[(size_t)n * MAX_PLACE + tid];
            if (q.frame >= 0 && q.frame < F) {
                const cnl_letterbox_frame fr = frames[q.frame];
                // every comparison is written so that no sum can overflow
                const bool window = q.w >= 1 && q.h >= 1 && q.x0 >= 0 && q.y0 >= 0 && q.w <= fr.w && q.h <= fr.h && q.x0 <= fr.w - q.w && q.y0 <= fr.h - q.h;
                const bool rect = q.dw >= 4 && q.dh >= 1 && q.dx0 >= 0 && q.dy0 >= 0 && ((q.dx0 | q.dw) & 3) == 0 && q.dw <= width && q.dh <= height &&
                                  q.dx0 <= width - q.dw && q.dy0 <= height - q.dh;
                if (window && rect && fr.src) {
                    e.src = (const unsigned char*)fr.src + (size_t)q.y0 * fr.row_stride + (size_t)q.x0 * 3;
                    e.row_stride = fr.row_stride;
                    e.w = q.w;
                    e.h = q.h;
                    e.live = 1;
                    e.x0 = q.dx0;
                    e.y0 = q.dy0;
                    e.x1 = q.dx0 + q.dw;
                    e.y1 = q.dy0 + q.dh;
                    e.dw = q.dw;
                    e.dh = q.dh;
                    e.flip = q.flip != 0;
                    for (int k = 0; k < 12; ++k) e.m[k] = q.colour[k];
                }
            }
        }
        place[tid] = e;
    }
    if (tid < 64) {                              // the first wave: which holes touch this tile
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
    __syncthreads();

    for (int p = 0; p < MAX_PLACE; ++p) {
        const Placement& q = place[p];
        if (!q.live || q.x0 >= x_end || q.x1 <= x_begin || q.y0 >= row_end || q.y1 <= row_begin) continue;      // uniform
        const double scale_x = axis_scale(q.dw, q.w), scale_y = axis_scale(q.dh, q.h);
        const int c_begin = max(q.x0, x_begin), c_end = min(q.x1, x_end);
        for (int x = c_begin + tid; x < c_end; x += LB_THREADS) {
            const int dx = x - q.x0;
            col[p][x - x_begin] = column_entry<Source>(q.flip ? q.dw - 1 - dx : dx, scale_x, q.w);
        }
        if (tid < n_rows) {
            const int y = row_begin + tid;
            if (y >= q.y0 && y < q.y1) row[p][tid] = row_entry(y - q.y0, scale_y, q.h);
        }
    }
    __syncthreads();

    const unsigned touching = (unsigned)__builtin_amdgcn_readfirstlane((int)hole_mask);
    unsigned char* const canvas = out + (size_t)n * height * width * 3;
    const int items = n_rows * n_groups;
    for (int i = tid; i < items; i += LB_THREADS) {
        const int r = i / n_groups, g = i - r * n_groups;
        const int y = row_begin + r, x = x_begin + g * 4;
        int sel = -1;
#pragma unroll
        for (int p = MAX_PLACE - 1; p >= 0; --p) {             // the first live placement that holds the group (rectangles of a checked plan are disjoint)
            const Placement& q = place[p];
            if (q.live && y >= q.y0 && y < q.y1 && x >= q.x0 && x < q.x1) sel = p;
        }
        unsigned px[4];                          // pixel p's three channel bytes, channel c at bits 8c
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = fill;
        if (sel >= 0) {
            const Placement& q = place[sel];
            cnl_letterbox_frame window = {};
            window.src = q.src;
            window.h = q.h;
            window.w = q.w;
            window.row_stride = q.row_stride;
            const Source source(window, {});
            const int4 rc = row[sel][r];
            const int4 c01 = reinterpret_cast<const int4*>(col[sel])[g * 2], c23 = reinterpret_cast<const int4*>(col[sel])[g * 2 + 1];
            const int2 c4[4] = {make_int2(c01.x, c01.y), make_int2(c01.z, c01.w), make_int2(c23.x, c23.y), make_int2(c23.z, c23.w)};
            sample_group(source, rc, c4, px);
            int m[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) m[k] = q.m[k];
#pragma unroll
            for (int p = 0; p < 4; ++p) {        // |m| <= 32767 and |offset| <= 2^21 (the entry's contract): 3 * 255 * 32767 + 2^21 + 2^11 < 2^31
                const int R = (int)(px[p] & 255u), G = (int)((px[p] >> 8) & 255u), B = (int)((px[p] >> 16) & 255u);
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
                px[p] = v;
            }
        }
        for (unsigned left = touching; left; left &= left - 1) {
            const int4 h = hole[__builtin_ctz(left)];
            if (y >= h.y && y < h.w) {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (x + p >= h.x && x + p < h.z) px[p] = hole_fill;
            }
        }
        store_group<3>(reinterpret_cast<unsigned*>(canvas + ((size_t)y * width + (size_t)x) * 3), px);
    }
}

// one workgroup per canvas; placements in slot order, boxes in source order, in chunks of BOX_THREADS
__global__ __launch_bounds__(BOX_THREADS) void augment_boxes_kernel(const cnl_augment_placement* __restrict__ places, const int* __restrict__ n_place, int F,
                                                                    int max_place, const double* __restrict__ boxes, const long long* __restrict__ labels,
                                                                    const long long* __restrict__ ids, const int* __restrict__ count, int Gmax,
                                                                    double* __restrict__ out_boxes, long long* __restrict__ out_labels,
                                                                    long long* __restrict__ out_ids, int* __restrict__ out_count, int Gout, double min_area,
                                                                    double min_visibility) {
    __shared__ int wave_kept[BOX_THREADS / 64];
    const int n = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = min(max(n_place[n], 0), max_place);
    double* const ob = out_boxes + (size_t)n * Gout * 4;
    long long* const ol = out_labels + (size_t)n * Gout;
    long long* const oi = out_ids ? out_ids + (size_t)n * Gout : nullptr;
    int base = 0;                                // kept so far: uniform
    for (int p = 0; p < np; ++p) {
        const cnl_augment_placement q = places[(size_t)n * MAX_PLACE + p];       // uniform address: scalar loads
        if (q.frame < 0 || q.frame >= F || q.w < 1 || q.h < 1 || q.dw < 1 || q.dh < 1) continue;
        const int cnt = min(max(count[q.frame], 0), Gmax);
        const double dw = (double)q.dw, dh = (double)q.dh;
        const double sx = dw / (double)q.w, sy = dh / (double)q.h;
        const double x0 = (double)q.x0, y0 = (double)q.y0;
        for (int j0 = 0; j0 < cnt; j0 += BOX_THREADS) {
            const int j = j0 + tid;
            bool keep = false;
            double bx = 0, by = 0, bw = 0, bh = 0;
            long long label = 0, id = 0;
            if (j < cnt) {
                const size_t s = (size_t)q.frame * Gmax + j;
                const double x = boxes[s * 4], y = boxes[s * 4 + 1], w = boxes[s * 4 + 2], h = boxes[s * 4 + 3];
                label = labels[s];
                if (ids) id = ids[s];
                double u1 = (x - x0) * sx, u2 = (x + w - x0) * sx;
                const double v1 = (y - y0) * sy, v2 = (y + h - y0) * sy;
                if (q.flip) {
                    const double t = dw - u2;
                    u2 = dw - u1;
                    u1 = t;
                }
                const double full = (u2 - u1) * (v2 - v1);
                const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(w) && __builtin_isfinite(h) &&
                                    __builtin_isfinite(u1) && __builtin_isfinite(u2) && __builtin_isfinite(v1) && __builtin_isfinite(v2) &&
                                    __builtin_isfinite(full);
                if (finite) {
                    const double cu1 = fmin(fmax(u1, 0.0), dw), cu2 = fmin(fmax(u2, 0.0), dw);
                    const double cv1 = fmin(fmax(v1, 0.0), dh), cv2 = fmin(fmax(v2, 0.0), dh);
                    bw = cu2 - cu1;
                    bh = cv2 - cv1;
                    const double area = bw * bh;
                    keep = bw > 0.0 && bh > 0.0 && area >= min_area && area >= min_visibility * full && label >= 0;
                    bx = (double)q.dx0 + cu1;
                    by = (double)q.dy0 + cv1;
                }
            }
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
                    ob[(size_t)pos * 4] = bx;
                    ob[(size_t)pos * 4 + 1] = by;
                    ob[(size_t)pos * 4 + 2] = bw;
                    ob[(size_t)pos * 4 + 3] = bh;
                    ol[pos] = label;
                    if (oi) oi[pos] = id;
                }
            }
            base += total;
            __syncthreads();                     // wave_kept is rewritten by the next chunk
        }
    }
    base = min(base, Gout);
    for (int j = base + tid; j < Gout; j += BOX_THREADS) {     // slots beyond count[n] are exactly zero
        ob[(size_t)j * 4] = ob[(size_t)j * 4 + 1] = ob[(size_t)j * 4 + 2] = ob[(size_t)j * 4 + 3] = 0.0;
        ol[j] = 0;
        if (oi) oi[j] = 0;
    }
    if (tid == 0) out_count[n] = base;
}

static int check_plan(const char* entry, const void* places, const int32_t* n_place, int N, int F, int max_place) {
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "%s: N = %d outside 0..65535", entry, N);
    CNL_REQUIRE(F >= 0 && F <= 65535, CNL_E_BAD_ARG, "%s: F = %d outside 0..65535", entry, F);
    CNL_REQUIRE(max_place >= 1 && max_place <= MAX_PLACE, CNL_E_BAD_ARG, "%s: max_place = %d outside 1..%d", entry, max_place, MAX_PLACE);
    if (N == 0) return CNL_OK;                   // an empty batch is a no-op: its pointers are not looked at
    CNL_REQUIRE(places && n_place, CNL_E_BAD_ARG, "%s: null plan pointer", entry);
    CNL_REQUIRE(((uintptr_t)places & 7) == 0 && ((uintptr_t)n_place & 3) == 0, CNL_E_BAD_ARG, "%s: places must be 8-byte and n_place 4-byte aligned", entry);
    return CNL_OK;
}

}  // namespace cnl_augment

extern "C" int cnl_augment_u8(const void* frames, int32_t F, const void* places, const int32_t* n_place, int32_t max_place, const int32_t* holes,
                              uint8_t* out, int32_t N, int32_t height, int32_t width, uint32_t fill_rgba, uint32_t hole_fill_rgba, void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_u8";
    if (int e = check_plan(entry, places, n_place, N, F, max_place)) return e;
    CNL_REQUIRE(height >= 1 && height <= 32768 && width >= 4 && width <= 32768 && width % 4 == 0, CNL_E_BAD_ARG,
                "%s: canvas %d x %d needs a height in 1..32768 and a width in 4..32768 that is a multiple of 4", entry, height, width);
    CNL_REQUIRE((long)height * width * 3 <= 0x7fffffffL, CNL_E_BAD_ARG, "%s: one canvas exceeds 2 GiB", entry);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(out && (frames || F == 0), CNL_E_BAD_ARG, "%s: null pointer", entry);
    CNL_REQUIRE(((uintptr_t)frames & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)holes & 15) == 0, CNL_E_BAD_ARG,
                "%s: frames must be 8-byte, out 4-byte and holes 16-byte aligned", entry);
    const int groups = width / 4;
    const int tiles_x = (groups + LB_TILE_GROUPS - 1) / LB_TILE_GROUPS;
    const int groups_per_tile = (groups + tiles_x - 1) / tiles_x;            // equal tiles, as letterbox_kernel's launch
    const int row_blocks = (height + LB_ROWS - 1) / LB_ROWS;
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)(tiles_x * row_blocks), (unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream,
                       static_cast<const cnl_letterbox_frame*>(frames), F, static_cast<const cnl_augment_placement*>(places), n_place,
                       reinterpret_cast<const int4*>(holes), out, height, width, max_place, fill_rgba & 0xffffffu, hole_fill_rgba & 0xffffffu, tiles_x,
                       groups_per_tile);
    return cnl::check_launch("augment_kernel");
}

extern "C" int cnl_augment_boxes_f64(const void* places, const int32_t* n_place, int32_t max_place, int32_t N, int32_t F, const double* boxes,
                                     const int64_t* labels, const int64_t* ids, const int32_t* count, int32_t Gmax, double* out_boxes,
                                     int64_t* out_labels, int64_t* out_ids, int32_t* out_count, int32_t Gout, double min_area, double min_visibility,
                                     void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_boxes_f64";
    if (int e = check_plan(entry, places, n_place, N, F, max_place)) return e;
    CNL_REQUIRE(Gmax >= 1 && Gmax <= 65535, CNL_E_BAD_ARG, "%s: Gmax = %d outside 1..65535", entry, Gmax);
    CNL_REQUIRE(Gout >= max_place * Gmax, CNL_E_BAD_ARG, "%s: Gout = %d is smaller than max_place * Gmax = %d", entry, Gout, max_place * Gmax);
    CNL_REQUIRE(min_area == min_area && min_visibility == min_visibility, CNL_E_BAD_ARG, "%s: min_area or min_visibility is NaN", entry);
    CNL_REQUIRE((ids == nullptr) == (out_ids == nullptr), CNL_E_BAD_ARG, "%s: ids and out_ids are given together", entry);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(out_boxes && out_labels && out_count && (F == 0 || (boxes && labels && count)), CNL_E_BAD_ARG, "%s: null pointer", entry);
    CNL_REQUIRE(((uintptr_t)boxes & 7) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)ids & 7) == 0 && ((uintptr_t)count & 3) == 0 &&
                    ((uintptr_t)out_boxes & 7) == 0 && ((uintptr_t)out_labels & 7) == 0 && ((uintptr_t)out_ids & 7) == 0 && ((uintptr_t)out_count & 3) == 0,
                CNL_E_BAD_ARG, "%s: boxes, labels and ids must be 8-byte, counts 4-byte aligned", entry);
    hipLaunchKernelGGL(augment_boxes_kernel, dim3((unsigned)N), dim3(BOX_THREADS), 0, (hipStream_t)stream, static_cast<const cnl_augment_placement*>(places),
                       n_place, F, max_place, boxes, reinterpret_cast<const long long*>(labels), reinterpret_cast<const long long*>(ids), count, Gmax, out_boxes,
                       reinterpret_cast<long long*>(out_labels), reinterpret_cast<long long*>(out_ids), out_count, Gout, min_area, min_visibility);
    return cnl::check_launch("augment_boxes_kernel");
}
