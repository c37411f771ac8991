// letterbox.hip — the batch entry for frames of DIFFERENT sizes, from packed uint8 HWC frames or straight from YUV 4:2:0 video surfaces
// (NV12 / I420), and the way back for the decoded boxes.
//
//   letterbox_kernel<Source>   N frames (or windows of frames: tiles), each with its own size, -> one [N, height, width, C] canvas:
//                              keep-aspect bilinear resize (albumentations LongestMaxSize = cv2.resize INTER_LINEAR, the 8-bit fixed-point
//                              rule of preprocess.hip's resize_bilinear_u8_kernel, bit for bit) centred on a constant border
//                              (PadIfNeeded(position="center", border_mode=BORDER_CONSTANT)), in ONE launch that writes every canvas
//                              byte exactly once.  ONE body; what a source pixel is comes from the Source policy:
//       PackedSource<C>        cnl_letterbox_frame records: C-channel bytes, C in 1..4
//       Yuv420Source           cnl_yuv420_frame records: Y / U / V planes, converted to RGB on the resize's taps in registers by the
//                              integer rule of include/centernet_gfx950.h (OpenCV's cvtColor arithmetic, nearest chroma), so the RGB
//                              frame between the decoder and the network is never written; bit for bit PackedSource<3> on the
//                              converted frames
//   unletterbox_kernel         decoded boxes in canvas pixels -> each frame's own pixels, in place.
//   crop_records_kernel<Frame> boxes [N, k, 4] in frame pixels -> one window record per slot, made on the device; letterbox_kernel over
//                              those records is cnl_crop_boxes_u8: every detection cut out of its frame at one size.
//
// The reference does this on the host, one image at a time (configs/centernet.yaml val_data.transforms; datasets/inference.py carries
// original_height / original_width), and therefore validates at batch size 1.
//
// Decomposition of letterbox_kernel (a pure streaming kernel: 2 source rows read per output row, no reuse worth staging):
//   grid.y = record, grid.x = (block of LB_ROWS canvas rows) x (column tile of <= 1024 canvas columns).  A frame is never one workgroup's
//   job: a 1080p frame and a 7 x 5 frame in one batch cost the same number of equally sized workgroups (the canvas is what is tiled).
//   The record is read through a uniform pointer (scalar loads).  The per-column terms (the source column as the policy addresses it,
//   the two 11-bit weights) are the same for every row of a frame and the per-row terms for every column: both are computed once per
//   workgroup into LDS — fp64 multiply, floor and two roundings per COLUMN instead of per pixel — and read back as one 32-byte LDS read
//   per thread.  A thread owns 4 neighbouring canvas pixels = C whole 32-bit words (3 words at C = 3, one 16-byte store at C = 4):
//   width % 32 == 0 keeps every row word-aligned, so no byte store exists.
// A Source policy supplies: Frame (its record; both carry h, w, new_h, new_w, pad_top, pad_left), Params (kernel arguments of its own),
//   C, column(sx) (what the column table keeps for source column sx), load() (ALL loads of a thread's 4-pixel group, issued together
//   before the first is used) and taps() (pixel p's four tap values, channel c at bits 8c: upper-left, upper-right, lower-left,
//   lower-right).  The format is a template parameter: no branch on it exists at run time.
//   Packed: the two source pixels of a tap are one unaligned 8-byte load (sx*C .. +2C-1, the start pulled back so the load never leaves
//   the row; rows shorter than 8 bytes take byte loads): 8 loads per thread.  YUV: a tap is one Y byte load and its chroma sample (one
//   2-byte load for NV12's interleaved UV, two byte loads for I420): 32 / 48 loads per thread, 1.5 bytes per source pixel instead of 3.
//   Measured rates and what limits them: DESIGN.md §12, §15.
#include <algorithm>
#include <cstdlib>
#include "letterbox_sampling.h"   // the sampling rule itself (shared with augment.hip): axis_coef, the table entries, PackedSource, sample_group

#pragma clang fp contract(off)   // OpenCV rounds (dx + 0.5) * scale and the subtraction separately

namespace cnl_letterbox {

static_assert(sizeof(cnl_yuv420_frame) == 72, "cnl_yuv420_frame is 72 bytes");

// YUV 4:2:0 planes (cnl_yuv420_frame, 72 bytes): the record's window (x0, y0, h, w) lies inside the frame, and chroma is addressed in
// FRAME coordinates; the column table keeps the window column of the left tap
struct Yuv420Source {
    static constexpr int C = 3;
    typedef cnl_yuv420_frame Frame;
    struct Params {
        int y_off, cy, cvr, cvg, cug, cub;
    };
    struct Taps {
        int Y[4][4], UV[4][4];                   // [pixel][tap]; UV = U | V << 8
    };
    const Frame& f;
    const Params& k;
    const gbytes yp, up, vp;
    const bool interleaved;                      // NV12: U and V in one 2-byte load

    __device__ __forceinline__ Yuv420Source(const Frame& f, const Params& k)
        : f(f), k(k), yp((gbytes)f.y), up((gbytes)f.u), vp((gbytes)f.v),
          interleaved(f.c_step == 2 && f.v == (const void*)((const unsigned char*)f.u + 1)) {}
    static __device__ __forceinline__ int column(int sx) { return sx; }

    // a border pixel reads its row's first column; the caller drops it.  The right tap of the window's last column is the left tap
    // again: its weight a1 is 0 there.
    __device__ __forceinline__ void load(int y0, int y1, const int2 (&c4)[4], Taps& t) const {
        const int fy0 = f.y0 + y0, fy1 = f.y0 + y1;                     // the two source rows, in frame coordinates
        const gbytes y0r = yp + (size_t)fy0 * f.y_pitch, y1r = yp + (size_t)fy1 * f.y_pitch;
        const size_t c0r = (size_t)(fy0 >> 1) * f.c_pitch, c1r = (size_t)(fy1 >> 1) * f.c_pitch;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int sx = max(c4[p].x, 0);
            const int xl = f.x0 + sx, xr = f.x0 + min(sx + 1, f.w - 1);
            const int cl = (xl >> 1) * f.c_step, cr = (xr >> 1) * f.c_step;
            t.Y[p][0] = y0r[xl];
            t.Y[p][1] = y0r[xr];
            t.Y[p][2] = y1r[xl];
            t.Y[p][3] = y1r[xr];
            if (interleaved) {
                t.UV[p][0] = *(gpairs)(up + c0r + cl);
                t.UV[p][1] = *(gpairs)(up + c0r + cr);
                t.UV[p][2] = *(gpairs)(up + c1r + cl);
                t.UV[p][3] = *(gpairs)(up + c1r + cr);
            } else {
                t.UV[p][0] = up[c0r + cl] | (vp[c0r + cl] << 8);
                t.UV[p][1] = up[c0r + cr] | (vp[c0r + cr] << 8);
                t.UV[p][2] = up[c1r + cl] | (vp[c1r + cl] << 8);
                t.UV[p][3] = up[c1r + cr] | (vp[c1r + cr] << 8);
            }
        }
    }
    static __device__ __forceinline__ unsigned sat8(int v) { return (unsigned)min(max(v, 0), 255); }
    // one source pixel -> R | G << 8 | B << 16
    __device__ __forceinline__ unsigned yuv_to_rgb(int Y, int U, int V) const {
        const int yy = max(Y - k.y_off, 0) * k.cy + (1 << 19), u = U - 128, v = V - 128;
        return sat8((yy + k.cvr * v) >> 20) | (sat8((yy + k.cvg * v + k.cug * u) >> 20) << 8) | (sat8((yy + k.cub * u) >> 20) << 16);
    }
    __device__ __forceinline__ void taps(const Taps& t, int p, unsigned (&v)[4]) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = yuv_to_rgb(t.Y[p][q], t.UV[p][q] & 255, t.UV[p][q] >> 8);
    }
};

template <class Source, int ROWS>
__global__ __launch_bounds__(LB_THREADS) void letterbox_kernel(const typename Source::Frame* __restrict__ table, unsigned char* __restrict__ out,
                                                               int height, int width, typename Source::Params params, unsigned fill,
                                                               int tiles_x, int groups_per_tile) {
    constexpr int C = Source::C;
    // col: .x = Source::column of the left tap's source column (-1: border), .y = a0 | a1 << 16
    __shared__ __attribute__((aligned(16))) int2 col[LB_TILE_GROUPS * 4];
    __shared__ int4 row[ROWS];                   // .x = y0 (-1: border row), .y = y1, .z = b0, .w = b1
    static_assert(ROWS >= 1 && ROWS <= LB_THREADS, "one thread fills one row entry");
    const typename Source::Frame f = table[blockIdx.y];          // uniform address: scalar loads
    const int tile = (int)(blockIdx.x % (unsigned)tiles_x), rblk = (int)(blockIdx.x / (unsigned)tiles_x);
    const int groups = width >> 2;
    const int g_begin = tile * groups_per_tile, g_end = min(groups, g_begin + groups_per_tile);
    const int n_groups = g_end - g_begin;
    const int x_begin = g_begin * 4, n_cols = n_groups * 4;
    const int row_begin = rblk * ROWS, n_rows = min(ROWS, height - row_begin);

    const double scale_x = axis_scale(f.new_w, f.w), scale_y = axis_scale(f.new_h, f.h);
    for (int i = threadIdx.x; i < n_cols; i += LB_THREADS) {
        const int dx = x_begin + i - f.pad_left;
        col[i] = dx >= 0 && dx < f.new_w ? column_entry<Source>(dx, scale_x, f.w) : make_int2(-1, 0);
    }
    if ((int)threadIdx.x < n_rows) {
        const int dy = row_begin + (int)threadIdx.x - f.pad_top;
        row[threadIdx.x] = dy >= 0 && dy < f.new_h ? row_entry(dy, scale_y, f.h) : make_int4(-1, 0, 0, 0);
    }
    __syncthreads();

    const Source source(f, params);
    unsigned char* const canvas = out + (size_t)blockIdx.y * height * width * C;
    const int items = n_rows * n_groups;
    for (int i = threadIdx.x; i < items; i += LB_THREADS) {
        const int r = i / n_groups, g = i - r * n_groups;
        const int4 rc = row[r];
        unsigned px[4];                          // pixel p's C channel bytes, channel c at bits 8c
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = fill;
        if (rc.x >= 0) {
            const int4 c01 = reinterpret_cast<const int4*>(col)[g * 2], c23 = reinterpret_cast<const int4*>(col)[g * 2 + 1];
            const int2 c4[4] = {make_int2(c01.x, c01.y), make_int2(c01.z, c01.w), make_int2(c23.x, c23.y), make_int2(c23.z, c23.w)};
            sample_group(source, rc, c4, px);
        }
        store_group<C>(reinterpret_cast<unsigned*>(canvas + ((size_t)(row_begin + r) * width + (size_t)(g_begin + g) * 4) * C), px);
    }
}

// boxes [N, k, 4] (x1 y1 x2 y2) in canvas pixels -> the frame's own pixels, in place; one thread per box (one 16-byte load and store)
__global__ __launch_bounds__(256) void unletterbox_kernel(float4* __restrict__ boxes, const cnl_letterbox_frame* __restrict__ table, int N, int k,
                                                          int clip) {
    const long total = (long)N * k;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const cnl_letterbox_frame& f = table[t / k];
        const float sx = (float)f.new_w / (float)f.w, sy = (float)f.new_h / (float)f.h;
        const float pl = (float)f.pad_left, pt = (float)f.pad_top;
        float4 b = boxes[t];
        b.x = (b.x - pl) / sx;
        b.y = (b.y - pt) / sy;
        b.z = (b.z - pl) / sx;
        b.w = (b.w - pt) / sy;
        if (clip) {
            const float wf = (float)f.w, hf = (float)f.h;
            b.x = fminf(fmaxf(b.x, 0.f), wf);
            b.y = fminf(fmaxf(b.y, 0.f), hf);
            b.z = fminf(fmaxf(b.z, 0.f), wf);
            b.w = fminf(fmaxf(b.w, 0.f), hf);
        }
        boxes[t] = b;
    }
}

// ---- crops: cnl_crop_boxes_u8 = crop_records_kernel (boxes -> one record per slot, on the device) + letterbox_kernel over those records
// canvas rows per workgroup for crop canvases.  LB_ROWS = 8 leaves half of a workgroup's threads without an item on a 64-pixel-wide crop
// and rebuilds the fp64 column table 16 times per 128-row crop; measured candidates and the choice: DESIGN.md §16, tools/crop_bench.py
#ifndef CNL_CROP_ROWS
#define CNL_CROP_ROWS 32
#endif
constexpr int CROP_ROWS = CNL_CROP_ROWS;

struct CropRule {
    int k, C, crop_h, crop_w, keep_aspect;
    float pad, threshold;
};

// where a slot's window starts, in the record of its frame's type: a packed frame moves its pointer, a YUV frame names the origin
// (chroma is addressed in frame coordinates, so odd origins need nothing more)
__device__ __forceinline__ void set_origin(cnl_letterbox_frame& r, int x0, int y0, int C) {
    r.src = (const unsigned char*)r.src + (size_t)y0 * r.row_stride + (size_t)x0 * C;
}
__device__ __forceinline__ void set_origin(cnl_yuv420_frame& r, int x0, int y0, int) {
    r.x0 = x0;
    r.y0 = y0;
}
// clamp in float, then convert: a NaN becomes 0 and no magnitude overflows the conversion
__device__ __forceinline__ int clamp_to_int(float v, float limit) {
    v = v > 0.f ? v : 0.f;
    return (int)(v < limit ? v : limit);
}

// one thread per slot (n, j) of boxes [N, k, 4]; the window, live and target rules are those of include/centernet_gfx950.h, one fp32
// operation per step (fp contract is off in this file)
template <class Frame>
__global__ __launch_bounds__(256) void crop_records_kernel(const Frame* __restrict__ frames, const float4* __restrict__ boxes,
                                                           const float* __restrict__ scores, const int* __restrict__ count,
                                                           Frame* __restrict__ records, int4* __restrict__ windows, long total, CropRule q) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int n = (int)(t / q.k), j = (int)(t - (long)n * q.k);
    Frame r = frames[n];                         // the whole frame: h, w are its size
    const float4 b = boxes[t];
    const bool live = (!count || j < count[n]) && (!scores || scores[t] >= q.threshold) && __builtin_isfinite(b.x) &&
                      __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && __builtin_isfinite(b.w);
    const float W = (float)r.w, H = (float)r.h;
    const float bw = b.z - b.x, bh = b.w - b.y;
    const float px = q.pad * bw, py = q.pad * bh;
    const int x0 = clamp_to_int(floorf(b.x - px), W), xe = clamp_to_int(ceilf(b.z + px), W);
    const int y0 = clamp_to_int(floorf(b.y - py), H), ye = clamp_to_int(ceilf(b.w + py), H);
    const int w = xe - x0, h = ye - y0;
    int4 win = make_int4(0, 0, 0, 0);
    if (live && w >= 1 && h >= 1) {
        win = make_int4(x0, y0, w, h);
        set_origin(r, x0, y0, q.C);
        r.h = h;
        r.w = w;
        r.new_h = q.crop_h;
        r.new_w = q.crop_w;
        if (q.keep_aspect) {                     // letterbox_geometry's rule, in double
            const double ratio = fmin((double)q.crop_h / (double)h, (double)q.crop_w / (double)w);
            r.new_h = min(q.crop_h, max(1, (int)rint((double)h * ratio)));
            r.new_w = min(q.crop_w, max(1, (int)rint((double)w * ratio)));
        }
        r.pad_top = (q.crop_h - r.new_h) / 2;
        r.pad_left = (q.crop_w - r.new_w) / 2;
    } else {                                     // dead: every canvas pixel is border, and no size is 0 for the gather to divide by
        set_origin(r, 0, 0, q.C);
        r.h = r.w = r.new_h = r.new_w = 1;
        r.pad_top = q.crop_h;
        r.pad_left = q.crop_w;
    }
    r.reserved = 0;
    records[t] = r;
    windows[t] = win;
}

// what both gather entry points require of the canvas, and then (the YUV entry checks its coefficients in between) of the pointers;
// `entry` names the one that was called
static int check_canvas(const char* entry, int N, int height, int width, int C) {
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "%s: N = %d outside 0..65535", entry, N);
    CNL_REQUIRE(C >= 1 && C <= 4, CNL_E_BAD_ARG, "%s: C = %d outside 1..4", entry, C);
    CNL_REQUIRE(height > 0 && width > 0 && height % 32 == 0 && width % 32 == 0, CNL_E_BAD_ARG,
                "%s: canvas %d x %d is not a positive multiple of 32", entry, height, width);
    CNL_REQUIRE((long)height * width * C <= 0x7fffffffL, CNL_E_BAD_ARG, "%s: the canvas of one frame exceeds 2 GiB", entry);
    return CNL_OK;
}
// the six colour integers of a YUV entry -> the kernel's Params, refused where the 32-bit conversion arithmetic could overflow
static int check_coefficients(const char* entry, const int32_t* coef, Yuv420Source::Params& k) {
    CNL_REQUIRE(coef, CNL_E_BAD_ARG, "%s: null coefficients", entry);
    k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    const long chroma = std::max(std::max(std::labs((long)k.cvr), std::labs((long)k.cvg) + std::labs((long)k.cug)), std::labs((long)k.cub));
    CNL_REQUIRE(k.y_off >= 0 && k.y_off <= 255 && k.cy >= 0 && 255L * k.cy + (1L << 19) + 128L * chroma < (1L << 31), CNL_E_UNSUPPORTED,
                "%s: coefficients {%d, %d, %d, %d, %d, %d} can overflow 32-bit arithmetic", entry, k.y_off, k.cy, k.cvr, k.cvg, k.cug, k.cub);
    return CNL_OK;
}
static int check_pointers(const char* entry, const void* table, const uint8_t* out, int N) {
    if (N == 0) return CNL_OK;                   // an empty batch is a no-op: its pointers are not looked at
    CNL_REQUIRE(table && out, CNL_E_BAD_ARG, "%s: null pointer", entry);
    CNL_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)out & 3) == 0, CNL_E_BAD_ARG, "%s: table must be 8-byte and out 4-byte aligned", entry);
    return CNL_OK;
}

// after the checks; `kernel` is the name a launch error is reported under.  ROWS = canvas rows per workgroup: LB_ROWS for the network-sized
// canvases of the two letterbox entries, CROP_ROWS for the small canvases of cnl_crop_boxes_u8
template <class Source, int ROWS = LB_ROWS>
static int launch(const char* kernel, const void* table, uint8_t* out, int N, int height, int width, typename Source::Params params, unsigned fill,
                  void* stream) {
    if (N == 0) return CNL_OK;
    const int groups = width / 4;
    const int tiles_x = (groups + LB_TILE_GROUPS - 1) / LB_TILE_GROUPS;
    const int groups_per_tile = (groups + tiles_x - 1) / tiles_x;           // equal tiles: 1088 columns = 2 x 136 groups, not 256 + 16
    const int row_blocks = (height + ROWS - 1) / ROWS;
    hipLaunchKernelGGL((letterbox_kernel<Source, ROWS>), dim3((unsigned)(tiles_x * row_blocks), (unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream,
                       static_cast<const typename Source::Frame*>(table), out, height, width, params, fill, tiles_x, groups_per_tile);
    return cnl::check_launch(kernel);
}

// both launches of cnl_crop_boxes_u8, after the checks; the gather runs in chunks of grid.y's limit
template <class Source>
static int crop(const void* frames, const float* boxes, const float* scores, const int32_t* count, void* records, int32_t* windows, uint8_t* out,
                long total, const CropRule& q, typename Source::Params params, unsigned fill, void* stream) {
    typedef typename Source::Frame Frame;
    hipLaunchKernelGGL(crop_records_kernel<Frame>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const Frame*>(frames), reinterpret_cast<const float4*>(boxes), scores, count, static_cast<Frame*>(records),
                       reinterpret_cast<int4*>(windows), total, q);
    if (int e = cnl::check_launch("crop_records_kernel")) return e;
    const size_t crop_bytes = (size_t)q.crop_h * q.crop_w * Source::C;
    for (long first = 0; first < total; first += 65535) {
        const int n = (int)std::min(65535L, total - first);
        if (int e = launch<Source, CROP_ROWS>("letterbox_kernel", static_cast<const Frame*>(records) + first, out + (size_t)first * crop_bytes, n,
                                              q.crop_h, q.crop_w, params, fill, stream))
            return e;
    }
    return CNL_OK;
}

}  // namespace cnl_letterbox

extern "C" int cnl_letterbox_bilinear_u8(const void* table, uint8_t* out, int32_t N, int32_t height, int32_t width, int32_t C,
                                         uint32_t fill_rgba, void* stream) {
    using namespace cnl_letterbox;
    if (int e = check_canvas("cnl_letterbox_bilinear_u8", N, height, width, C)) return e;
    if (int e = check_pointers("cnl_letterbox_bilinear_u8", table, out, N)) return e;
    switch (C) {
        case 1: return launch<PackedSource<1>>("letterbox_kernel", table, out, N, height, width, {}, fill_rgba, stream);
        case 2: return launch<PackedSource<2>>("letterbox_kernel", table, out, N, height, width, {}, fill_rgba, stream);
        case 3: return launch<PackedSource<3>>("letterbox_kernel", table, out, N, height, width, {}, fill_rgba, stream);
        default: return launch<PackedSource<4>>("letterbox_kernel", table, out, N, height, width, {}, fill_rgba, stream);
    }
}

extern "C" int cnl_letterbox_yuv420_u8(const void* table, uint8_t* out, int32_t N, int32_t height, int32_t width, const int32_t* coef,
                                       uint32_t fill_rgba, void* stream) {
    using namespace cnl_letterbox;
    if (int e = check_canvas("cnl_letterbox_yuv420_u8", N, height, width, 3)) return e;
    Yuv420Source::Params k;
    if (int e = check_coefficients("cnl_letterbox_yuv420_u8", coef, k)) return e;
    if (int e = check_pointers("cnl_letterbox_yuv420_u8", table, out, N)) return e;
    // the message keeps the name this launch has always been reported under; the kernel is letterbox_kernel<Yuv420Source>
    return launch<Yuv420Source>("letterbox_yuv420_kernel", table, out, N, height, width, k, fill_rgba, stream);
}

extern "C" int cnl_unletterbox_boxes_f32(float* boxes, const void* table, int32_t N, int32_t k, int32_t clip, void* stream) {
    CNL_REQUIRE(N >= 0 && k >= 0, CNL_E_BAD_ARG, "cnl_unletterbox_boxes_f32: negative N or k");
    if (N == 0 || k == 0) return CNL_OK;
    CNL_REQUIRE(boxes && table, CNL_E_BAD_ARG, "cnl_unletterbox_boxes_f32: null pointer");
    CNL_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)table & 7) == 0, CNL_E_BAD_ARG,
                "cnl_unletterbox_boxes_f32: boxes must be 16-byte and table 8-byte aligned");
    const long total = (long)N * k;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(cnl_letterbox::unletterbox_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(boxes), static_cast<const cnl_letterbox_frame*>(table), N, k, clip);
    return cnl::check_launch("unletterbox_kernel");
}

extern "C" int cnl_crop_boxes_u8(const void* frames, const float* boxes, const float* scores, float score_threshold, const int32_t* count, int32_t N,
                                 int32_t k, int32_t C, const int32_t* coef, float pad, int32_t keep_aspect, void* records, int32_t* windows,
                                 uint8_t* out, int32_t crop_h, int32_t crop_w, uint32_t fill_rgba, void* stream) {
    using namespace cnl_letterbox;
    CNL_REQUIRE(N >= 0 && k >= 0, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: negative N or k");
    const long total = (long)N * k;
    CNL_REQUIRE(total <= 0x7fffffffL, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: N * k = %ld slots exceed 2^31 - 1", total);
    CNL_REQUIRE(C >= 1 && C <= 4, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: C = %d outside 1..4", C);
    CNL_REQUIRE(!coef || C == 3, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: YUV frames give C = 3 crops, not C = %d", C);
    CNL_REQUIRE(crop_h >= 1 && crop_w >= 4 && crop_w % 4 == 0, CNL_E_BAD_ARG,
                "cnl_crop_boxes_u8: crop %d x %d needs a height >= 1 and a width that is a positive multiple of 4", crop_h, crop_w);
    CNL_REQUIRE((long)crop_h * crop_w * C <= 0x7fffffffL, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: one crop exceeds 2 GiB");
    CNL_REQUIRE(__builtin_isfinite(pad) && pad >= 0.f, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: pad = %g must be finite and >= 0", (double)pad);
    CNL_REQUIRE(!scores || score_threshold == score_threshold, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: score_threshold is NaN");
    Yuv420Source::Params yuv = {};
    if (coef)
        if (int e = check_coefficients("cnl_crop_boxes_u8", coef, yuv)) return e;
    if (total == 0) return CNL_OK;               // no slots: the pointers are not looked at
    CNL_REQUIRE(frames && boxes && records && windows && out, CNL_E_BAD_ARG, "cnl_crop_boxes_u8: null pointer");
    CNL_REQUIRE(((uintptr_t)frames & 7) == 0 && ((uintptr_t)records & 7) == 0 && ((uintptr_t)boxes & 15) == 0 && ((uintptr_t)windows & 15) == 0 &&
                    ((uintptr_t)out & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)count & 3) == 0,
                CNL_E_BAD_ARG, "cnl_crop_boxes_u8: frames and records must be 8-byte, boxes and windows 16-byte, out, scores and count 4-byte aligned");
    const CropRule q = {k, C, crop_h, crop_w, keep_aspect != 0, pad, score_threshold};
    if (coef) return crop<Yuv420Source>(frames, boxes, scores, count, records, windows, out, total, q, yuv, fill_rgba, stream);
    switch (C) {
        case 1: return crop<PackedSource<1>>(frames, boxes, scores, count, records, windows, out, total, q, {}, fill_rgba, stream);
        case 2: return crop<PackedSource<2>>(frames, boxes, scores, count, records, windows, out, total, q, {}, fill_rgba, stream);
        case 3: return crop<PackedSource<3>>(frames, boxes, scores, count, records, windows, out, total, q, {}, fill_rgba, stream);
        default: return crop<PackedSource<4>>(frames, boxes, scores, count, records, windows, out, total, q, {}, fill_rgba, stream);
    }
}
