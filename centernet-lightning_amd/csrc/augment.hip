// augment.hip — the training augmentation of a batch on the device: the reference's albumentations Compose (HorizontalFlip,
// RandomResizedCrop, ColorJitter, Cutout; datasets/builder.py::parse_transforms, one image at a time in DataLoader workers) and the batch-level
// Mosaic that datasets/transforms.py declares and never wrote, as a deterministic function of a PLAN the host drew.
//
//   augment_kernel        up to four placements per canvas (a window of a source frame -> a rectangle of the canvas), each mirrored or not and
//                         with its own Q12 colour matrix, then the holes: [N, height, width, 3] u8 in ONE launch that writes every canvas byte
//                         exactly once (no memset, no atomics).  The sampling rule is letterbox_kernel's, from the one copy in
//                         letterbox_sampling.h: a placement without flip, colour or holes is bit for bit cnl_letterbox_bilinear_u8.
//   boxes_kernel<WindowMap> the targets through the same plan in float64, one rounding per operation (fp contract is off), filtered by
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
// The colour step, the holes, the box rule from `full` on and the compaction are augment_common.h's, shared with augment_warp.hip.
#include "augment_common.h"

#pragma clang fp contract(off)   // the sampling rule and the box rule round every operation on its own

namespace cnl_augment {

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
                const bool rect = rect_ok(q.dx0, q.dy0, q.dw, q.dh, width, height);
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
    if (tid < 64) find_holes(holes, n, tid, width, height, x_begin, x_end, row_begin, row_end, hole, hole_mask);      // the first wave
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
            for (int p = 0; p < 4; ++p) px[p] = colour_step(m, px[p]);
        }
        punch(touching, hole, y, x, hole_fill, px);
        store_group<3>(reinterpret_cast<unsigned*>(canvas + ((size_t)y * width + (size_t)x) * 3), px);
    }
}

// the box rule up to `full` for one placement: scale, map the two corners, mirror (boxes_kernel of augment_common.h does the rest)
struct WindowMap {
    typedef cnl_augment_placement Record;
    const double dw, sx, sy, x0, y0;
    const int flip;
    static __device__ __forceinline__ bool live(const Record& q, int F) { return q.frame >= 0 && q.frame < F && q.w >= 1 && q.h >= 1 && q.dw >= 1 && q.dh >= 1; }
    __device__ __forceinline__ WindowMap(const Record& q)
        : dw((double)q.dw), sx((double)q.dw / (double)q.w), sy((double)q.dh / (double)q.h), x0((double)q.x0), y0((double)q.y0), flip(q.flip) {}
    // -> whether everything the box was mapped to is finite
    __device__ __forceinline__ bool extent(double x, double y, double w, double h, double& u1, double& u2, double& v1, double& v2) const {
        u1 = (x - x0) * sx;
        u2 = (x + w - x0) * sx;
        v1 = (y - y0) * sy;
        v2 = (y + h - y0) * sy;
        if (flip) {
            const double t = dw - u2;
            u2 = dw - u1;
            u1 = t;
        }
        return __builtin_isfinite(u1) && __builtin_isfinite(u2) && __builtin_isfinite(v1) && __builtin_isfinite(v2);
    }
};

}  // namespace cnl_augment

extern "C" int cnl_augment_u8(const void* frames, int32_t F, const void* places, const int32_t* n_place, int32_t max_place, const int32_t* holes,
                              uint8_t* out, int32_t N, int32_t height, int32_t width, uint32_t fill_rgba, uint32_t hole_fill_rgba, void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_u8";
    if (int e = check_plan(entry, places, n_place, N, F, max_place)) return e;
    if (int e = check_canvas(entry, frames, F, holes, out, N, height, width)) return e;
    if (N == 0) return CNL_OK;
    const CanvasGrid grid(height, width);
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)(grid.tiles_x * grid.row_blocks), (unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream,
                       static_cast<const cnl_letterbox_frame*>(frames), F, static_cast<const cnl_augment_placement*>(places), n_place,
                       reinterpret_cast<const int4*>(holes), out, height, width, max_place, fill_rgba & 0xffffffu, hole_fill_rgba & 0xffffffu, grid.tiles_x,
                       grid.groups_per_tile);
    return cnl::check_launch("augment_kernel");
}

extern "C" int cnl_augment_boxes_f64(const void* places, const int32_t* n_place, int32_t max_place, int32_t N, int32_t F, const double* boxes,
                                     const int64_t* labels, const int64_t* ids, const int32_t* count, int32_t Gmax, double* out_boxes,
                                     int64_t* out_labels, int64_t* out_ids, int32_t* out_count, int32_t Gout, double min_area, double min_visibility,
                                     void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_boxes_f64";
    if (int e = check_plan(entry, places, n_place, N, F, max_place)) return e;
    if (int e = check_boxes(entry, N, F, max_place, boxes, labels, ids, count, Gmax, out_boxes, out_labels, out_ids, out_count, Gout, min_area, min_visibility))
        return e;
    if (N == 0) return CNL_OK;
    hipLaunchKernelGGL(boxes_kernel<WindowMap>, dim3((unsigned)N), dim3(BOX_THREADS), 0, (hipStream_t)stream, static_cast<const cnl_augment_placement*>(places),
                       n_place, F, max_place, boxes, reinterpret_cast<const long long*>(labels), reinterpret_cast<const long long*>(ids), count, Gmax, out_boxes,
                       reinterpret_cast<long long*>(out_labels), reinterpret_cast<long long*>(out_ids), out_count, Gout, min_area, min_visibility);
    return cnl::check_launch("boxes_kernel<WindowMap>");
}
