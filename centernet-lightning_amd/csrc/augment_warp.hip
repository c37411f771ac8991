// augment_warp.hip — the affine training augmentation of a batch on the device: albumentations' Affine (scale, rotate, shear,
// translate), RandomResizedCrop / RandomCrop / SmallestMaxSize and HorizontalFlip composed by the host into ONE map per placement, so that every
// canvas pixel is resampled once (albumentations resamples twice: Affine, then the crop).
//
//   warp_kernel            up to four placements per canvas (an affine image of a source frame inside a rectangle of the canvas, clipped to a
//                          window of the frame, `border` outside it), each with its own Q12 colour matrix, then the holes: [N, height, width, 3]
//                          u8 in ONE launch that writes every canvas byte exactly once (no memset, no atomics).  The sampling rule is the header's
//                          Q20 inverse-map rule, all in integers: not cv2.warpAffine's and not the letterbox rule.
//   boxes_kernel<AffineMap> the targets through the placement's forward map in float64 (the enclosing box of the four mapped corners), then
//                          augment_common.h's clip, keep rule and stable compaction.
//
// Decomposition of warp_kernel: augment_kernel's.  grid.y = canvas, grid.x = (block of LB_ROWS canvas rows) x (column tile of <= 1024 columns);
// the first four threads turn the canvas's records into descriptors in LDS, the first wave finds the holes of the tile by one ballot; a thread
// owns 4 neighbouring pixels = three whole 32-bit words, and a group has ONE placement or none.  A rotated placement has no column and row tables:
// in their place the row terms inv[1] * dy + inv[2] and inv[4] * dy + inv[5] of every (placement, row of the block) are computed once, in LDS,
// and a thread steps inv[0] and inv[3] over its four pixels.  Per pixel two unaligned 8-byte loads, each the left and the right tap of one
// source row (PackedSource<3>'s load); the load offset is clamped into [0, 3 * fw - 8] of that frame row and the wanted six bytes are shifted
// into place, frames with rows shorter than 8 bytes are read bytewise, and a pixel whose four taps all lie outside the window reads nothing.
#include "augment_common.h"

#pragma clang fp contract(off)   // the box rule rounds every operation on its own

namespace cnl_augment {

static_assert(sizeof(cnl_warp_placement) == 192, "cnl_warp_placement is 192 bytes");
static_assert(offsetof(cnl_warp_placement, colour) == 40 && offsetof(cnl_warp_placement, inv) == 88 && offsetof(cnl_warp_placement, fwd) == 136,
              "cnl_warp_placement's layout");

constexpr long long INV_LINEAR_MAX = 1ll << 30, INV_OFFSET_MAX = 1ll << 44;

__device__ __forceinline__ bool inv_ok(const cnl_warp_placement& q) {
    const long long a = INV_LINEAR_MAX, b = INV_OFFSET_MAX;
    return q.inv[0] >= -a && q.inv[0] <= a && q.inv[1] >= -a && q.inv[1] <= a && q.inv[3] >= -a && q.inv[3] <= a && q.inv[4] >= -a && q.inv[4] <= a &&
           q.inv[2] >= -b && q.inv[2] <= b && q.inv[5] >= -b && q.inv[5] <= b;
}

// one placement as the workgroup uses it
struct WarpPlace {
    const void* src;                 // the FRAME's first pixel
    int row_stride, row_bytes;       // of the frame; row_bytes = 3 * frame width
    int live, pad;
    int wx0, wy0, wx1, wy1;          // the clip window in frame pixels, [wx0, wx1) x [wy0, wy1), inside the frame
    int x0, y0, x1, y1;              // the rectangle in canvas pixels, [x0, x1) x [y0, y1)
    long long ix, iy;                // inv[0], inv[3]: the step of X and Y per canvas column
    int m[12];                       // Q12 colour matrix
};

// the six bytes (left tap, right tap) of source columns sx, sx + 1 in the frame row `row` as bits 0..47: bytes that lie outside the row are
// zero (the caller replaces such taps by the border).  -1 <= sx <= frame width - 1.
__device__ __forceinline__ unsigned long long load_taps(gbytes row, int sx, int row_bytes) {
    const int want = sx * 3;                     // -3 .. row_bytes - 3
    if (row_bytes >= 8) {
        const int o = min(max(want, 0), row_bytes - 8);      // the 8 bytes [o, o + 8) are inside the row
        const unsigned long long t = *(gwords)(row + o);
        return want < 0 ? t << 24 : t >> ((want - o) * 8);   // want - o <= 5
    }
    unsigned long long t = 0;
    for (int b = 0; b < 6; ++b) {
        const int at = want + b;
        if (at >= 0 && at < row_bytes) t |= (unsigned long long)row[at] << (8 * b);
    }
    return t;
}

__global__ __launch_bounds__(LB_THREADS) void warp_kernel(const cnl_letterbox_frame* __restrict__ frames, int F, const cnl_warp_placement* __restrict__ places,
                                                          const int* __restrict__ n_place, const int4* __restrict__ holes, unsigned char* __restrict__ out,
                                                          int height, int width, int max_place, unsigned fill, unsigned hole_fill, unsigned border, int tiles_x,
                                                          int groups_per_tile) {
    __shared__ WarpPlace place[MAX_PLACE];
    __shared__ longlong2 row_term[MAX_PLACE][LB_ROWS];       // .x = inv[1] * dy + inv[2], .y = inv[4] * dy + inv[5] of the block's rows
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

    // threads 64 .. 64 + MAX_PLACE * LB_ROWS - 1 (the second wave) each read one record's row coefficients themselves: no barrier between
    // the descriptors and the row terms.  A term of a record that is not live is never read.
    if (tid < MAX_PLACE) {
        WarpPlace e = {};
        const int np = min(max(n_place[n], 0), max_place);
        if (tid < np) {
            const cnl_warp_placement q = places[(size_t)n * MAX_PLACE + tid];
            if (q.frame >= 0 && q.frame < F) {
                const cnl_letterbox_frame fr = frames[q.frame];
                // every comparison is written so that no sum can overflow
                const bool window = q.w >= 1 && q.h >= 1 && q.x0 >= 0 && q.y0 >= 0 && q.w <= fr.w && q.h <= fr.h && q.x0 <= fr.w - q.w && q.y0 <= fr.h - q.h;
                if (window && rect_ok(q.dx0, q.dy0, q.dw, q.dh, width, height) && inv_ok(q) && fr.src) {
                    e.src = fr.src;
                    e.row_stride = fr.row_stride;
                    e.row_bytes = fr.w * 3;
                    e.live = 1;
                    e.wx0 = q.x0;
                    e.wy0 = q.y0;
                    e.wx1 = q.x0 + q.w;
                    e.wy1 = q.y0 + q.h;
                    e.x0 = q.dx0;
                    e.y0 = q.dy0;
                    e.x1 = q.dx0 + q.dw;
                    e.y1 = q.dy0 + q.dh;
                    e.ix = q.inv[0];
                    e.iy = q.inv[3];
                    for (int k = 0; k < 12; ++k) e.m[k] = q.colour[k];
                }
            }
        }
        place[tid] = e;
    } else if (tid >= 64 && tid < 64 + MAX_PLACE * LB_ROWS) {
        const int p = (tid - 64) / LB_ROWS, r = (tid - 64) % LB_ROWS;
        longlong2 t = make_longlong2(0, 0);
        if (p < min(max(n_place[n], 0), max_place)) {
            const cnl_warp_placement* q = places + (size_t)n * MAX_PLACE + p;
            const long long dy = (long long)(row_begin + r) - q->dy0;
            // |inv[1]|, |inv[4]| <= 2^30 and |dy| < 2^32, |inv[2]|, |inv[5]| <= 2^44 for a live record; any other record's term wraps and is unused
            t.x = (long long)((unsigned long long)q->inv[1] * (unsigned long long)dy + (unsigned long long)q->inv[2]);
            t.y = (long long)((unsigned long long)q->inv[4] * (unsigned long long)dy + (unsigned long long)q->inv[5]);
        }
        row_term[p][r] = t;
    }
    if (tid < 64) find_holes(holes, n, tid, width, height, x_begin, x_end, row_begin, row_end, hole, hole_mask);      // the first wave
    __syncthreads();

    const unsigned touching = (unsigned)__builtin_amdgcn_readfirstlane((int)hole_mask);
    unsigned char* const canvas = out + (size_t)n * height * width * 3;
    const int items = n_rows * n_groups;
    for (int i = tid; i < items; i += LB_THREADS) {
        const int r = i / n_groups, g = i - r * n_groups;
        const int y = row_begin + r, x = x_begin + g * 4;
        int sel = -1;
#pragma unroll
        for (int p = MAX_PLACE - 1; p >= 0; --p) {             // the first live placement that holds the group: the lower slot wins
            const WarpPlace& q = place[p];
            if (q.live && y >= q.y0 && y < q.y1 && x >= q.x0 && x < q.x1) sel = p;
        }
        unsigned px[4];                          // pixel p's three channel bytes, channel c at bits 8c
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = fill;
        if (sel >= 0) {
            const WarpPlace& q = place[sel];
            const gbytes src = (gbytes)q.src;
            const int row_stride = q.row_stride, row_bytes = q.row_bytes;
            const int wx0 = q.wx0, wy0 = q.wy0, wx1 = q.wx1, wy1 = q.wy1;
            const long long ix = q.ix, iy = q.iy;
            const longlong2 rt = row_term[sel][r];
            // live: |ix * dx| < 2^30 * 2^15, |row term| < 2^30 * 2^15 + 2^44: every sum below stays under 2^47
            long long X = ix * (long long)(x - q.x0) + rt.x, Y = iy * (long long)(x - q.x0) + rt.y;
            unsigned long long t0[4], t1[4];     // per pixel, upper / lower source row; bytes 0..2: left tap, 3..5: right tap
            int sxs[4], sys[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const long long sx64 = X >> 20, sy64 = Y >> 20;
                // far outside is outside: clamp to one position beyond the window's reach, so that the 32-bit tests below are exact
                const int sx = (int)min(max(sx64, (long long)-2), (long long)wx1), sy = (int)min(max(sy64, (long long)-2), (long long)wy1);
                sxs[p] = sx;
                sys[p] = sy;
                const bool in_x = sx + 1 >= wx0 && sx < wx1, in_y0 = sy >= wy0 && sy < wy1, in_y1 = sy + 1 >= wy0 && sy + 1 < wy1;
                t0[p] = t1[p] = 0;
                // in_x: -1 <= sx <= frame width - 1; in_y0 / in_y1: that row is a row of the frame
                if (in_x && in_y0) t0[p] = load_taps(src + (size_t)sy * row_stride, sx, row_bytes);
                if (in_x && in_y1) t1[p] = load_taps(src + (size_t)(sy + 1) * row_stride, sx, row_bytes);
                X += ix;
                Y += iy;
            }
            X -= 4 * ix;
            Y -= 4 * iy;
            int m[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) m[k] = q.m[k];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int sx = sxs[p], sy = sys[p];
                const int a1 = (int)(X >> 9) & 2047, a0 = 2048 - a1, b1 = (int)(Y >> 9) & 2047, b0 = 2048 - b1;
                const bool x_l = sx >= wx0 && sx < wx1, x_r = sx + 1 >= wx0 && sx + 1 < wx1;
                const bool y_u = sy >= wy0 && sy < wy1, y_d = sy + 1 >= wy0 && sy + 1 < wy1;
                const unsigned t00 = x_l && y_u ? (unsigned)t0[p] : border, t10 = x_r && y_u ? (unsigned)(t0[p] >> 24) : border;
                const unsigned t01 = x_l && y_d ? (unsigned)t1[p] : border, t11 = x_r && y_d ? (unsigned)(t1[p] >> 24) : border;
                unsigned v4 = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int t = (int)((t00 >> (8 * c)) & 255u) * a0 + (int)((t10 >> (8 * c)) & 255u) * a1;
                    const int u = (int)((t01 >> (8 * c)) & 255u) * a0 + (int)((t11 >> (8 * c)) & 255u) * a1;
                    v4 |= (unsigned)((t * b0 + u * b1 + (1 << 21)) >> 22) << (8 * c);      // 255 * 2^22 + 2^21 < 2^31; 0..255 without a clamp
                }
                px[p] = colour_step(m, v4);
                X += ix;
                Y += iy;
            }
        }
        punch(touching, hole, y, x, hole_fill, px);
        store_group<3>(reinterpret_cast<unsigned*>(canvas + ((size_t)y * width + (size_t)x) * 3), px);
    }
}

// the box rule up to `full` for one placement: the four corners through the forward map, then their enclosing box
struct AffineMap {
    typedef cnl_warp_placement Record;
    double f[6];
    static __device__ __forceinline__ bool live(const Record& q, int F) {
        return q.frame >= 0 && q.frame < F && q.w >= 1 && q.h >= 1 && q.dw >= 1 && q.dh >= 1 && inv_ok(q);
    }
    __device__ __forceinline__ AffineMap(const Record& q) {
        for (int k = 0; k < 6; ++k) f[k] = q.fwd[k];
    }
    // -> whether everything the box was mapped to is finite
    __device__ __forceinline__ bool extent(double x, double y, double w, double h, double& u1, double& u2, double& v1, double& v2) const {
        const double xe = x + w, ye = y + h;
        const double ua = (f[0] * x + f[1] * y) + f[2], va = (f[3] * x + f[4] * y) + f[5];
        const double ub = (f[0] * xe + f[1] * y) + f[2], vb = (f[3] * xe + f[4] * y) + f[5];
        const double uc = (f[0] * x + f[1] * ye) + f[2], vc = (f[3] * x + f[4] * ye) + f[5];
        const double ud = (f[0] * xe + f[1] * ye) + f[2], vd = (f[3] * xe + f[4] * ye) + f[5];
        u1 = fmin(fmin(fmin(ua, ub), uc), ud);
        u2 = fmax(fmax(fmax(ua, ub), uc), ud);
        v1 = fmin(fmin(fmin(va, vb), vc), vd);
        v2 = fmax(fmax(fmax(va, vb), vc), vd);
        return __builtin_isfinite(ua) && __builtin_isfinite(ub) && __builtin_isfinite(uc) && __builtin_isfinite(ud) && __builtin_isfinite(va) &&
               __builtin_isfinite(vb) && __builtin_isfinite(vc) && __builtin_isfinite(vd);
    }
};

}  // namespace cnl_augment

extern "C" int cnl_augment_warp_u8(const void* frames, int32_t F, const void* places, const int32_t* n_place, int32_t max_place, const int32_t* holes,
                                   uint8_t* out, int32_t N, int32_t height, int32_t width, uint32_t fill_rgba, uint32_t hole_fill_rgba, uint32_t border_rgba,
                                   void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_warp_u8";
    if (int e = check_plan(entry, places, n_place, N, F, max_place)) return e;
    if (int e = check_canvas(entry, frames, F, holes, out, N, height, width)) return e;
    if (N == 0) return CNL_OK;
    const CanvasGrid grid(height, width);
    hipLaunchKernelGGL(warp_kernel, dim3((unsigned)(grid.tiles_x * grid.row_blocks), (unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream,
                       static_cast<const cnl_letterbox_frame*>(frames), F, static_cast<const cnl_warp_placement*>(places), n_place,
                       reinterpret_cast<const int4*>(holes), out, height, width, max_place, fill_rgba & 0xffffffu, hole_fill_rgba & 0xffffffu,
                       border_rgba & 0xffffffu, grid.tiles_x, grid.groups_per_tile);
    return cnl::check_launch("warp_kernel");
}

extern "C" int cnl_augment_warp_boxes_f64(const void* places, const int32_t* n_place, int32_t max_place, int32_t N, int32_t F, const double* boxes,
                                          const int64_t* labels, const int64_t* ids, const int32_t* count, int32_t Gmax, double* out_boxes,
                                          int64_t* out_labels, int64_t* out_ids, int32_t* out_count, int32_t Gout, double min_area, double min_visibility,
                                          void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_warp_boxes_f64";
    if (int e = check_plan(entry, places, n_place, N, F, max_place)) return e;
    if (int e = check_boxes(entry, N, F, max_place, boxes, labels, ids, count, Gmax, out_boxes, out_labels, out_ids, out_count, Gout, min_area, min_visibility))
        return e;
    if (N == 0) return CNL_OK;
    hipLaunchKernelGGL(boxes_kernel<AffineMap>, dim3((unsigned)N), dim3(BOX_THREADS), 0, (hipStream_t)stream, static_cast<const cnl_warp_placement*>(places),
                       n_place, F, max_place, boxes, reinterpret_cast<const long long*>(labels), reinterpret_cast<const long long*>(ids), count, Gmax, out_boxes,
                       reinterpret_cast<long long*>(out_labels), reinterpret_cast<long long*>(out_ids), out_count, Gout, min_area, min_visibility);
    return cnl::check_launch("boxes_kernel<AffineMap>");
}
