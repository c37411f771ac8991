// letterbox.hip — the batch entry for frames of DIFFERENT sizes, and the way back for the decoded boxes.
//
//   letterbox_kernel     N uint8 HWC frames, each with its own size, -> one [N, height, width, C] canvas: keep-aspect bilinear resize
//                        (albumentations LongestMaxSize = cv2.resize INTER_LINEAR, the 8-bit fixed-point rule of preprocess.hip's
//                        resize_bilinear_u8_kernel, bit for bit) centred on a constant border (PadIfNeeded(position="center",
//                        border_mode=BORDER_CONSTANT)), in ONE launch that writes every canvas byte exactly once.
//   unletterbox_kernel   decoded boxes in canvas pixels -> each frame's own pixels, in place.
//
// The reference does this on the host, one image at a time (configs/centernet.yaml val_data.transforms; datasets/inference.py carries
// original_height / original_width), and therefore validates at batch size 1.
//
// Decomposition of letterbox_kernel (a pure streaming kernel: 2 source rows read per output row, no reuse worth staging):
//   grid.y = frame, grid.x = (block of LB_ROWS canvas rows) x (column tile of <= 1024 canvas columns).  A frame is never one workgroup's
//   job: a 1080p frame and a 7 x 5 frame in one batch cost the same number of equally sized workgroups (the canvas is what is tiled).
//   The frame's record is read through a uniform pointer (scalar loads).  The per-column terms (source byte offset, the two 11-bit
//   weights) are the same for every row of a frame and the per-row terms for every column: both are computed once per workgroup into
//   LDS — fp64 multiply, floor and two roundings per COLUMN instead of per pixel — and read back as one 32-byte LDS read per thread.
//   A thread owns 4 neighbouring canvas pixels = C whole 32-bit words (3 words at C = 3, one 16-byte store at C = 4): width % 32 == 0
//   keeps every row word-aligned, so no byte store exists.  The two source pixels of a tap are one unaligned 8-byte load (sx*C .. +2C-1,
//   the start pulled back so the load never leaves the row; rows shorter than 8 bytes take byte loads), and the 8 loads of a thread's
//   group are issued together.  Measured rate and what limits it: DESIGN.md §12.
#include "cnl_common.h"

#pragma clang fp contract(off)   // OpenCV rounds (dx + 0.5) * scale and the subtraction separately

namespace cnl_letterbox {

constexpr int LB_THREADS = 256;
constexpr int LB_ROWS = 8;           // canvas rows per workgroup
constexpr int LB_TILE_GROUPS = 256;  // 4-pixel groups per column tile (1024 canvas columns)

typedef cnl_letterbox_frame Frame;   // include/centernet_gfx950.h (40 bytes)
typedef unsigned long long u64_unaligned __attribute__((aligned(1)));
// the frames' pointers come out of the table, so the compiler cannot tell their address space: name it (global_load, not flat_load)
typedef const __attribute__((address_space(1))) unsigned char* gbytes;
typedef const __attribute__((address_space(1))) u64_unaligned* gwords;

// resize_bilinear_u8_kernel's coefficient rule for one axis position
__device__ __forceinline__ void axis_coef(int d, double scale, int& s, float& f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}

template <int C>
__global__ __launch_bounds__(LB_THREADS) void letterbox_kernel(const Frame* __restrict__ table, unsigned char* __restrict__ out, int height,
                                                               int width, unsigned fill, int tiles_x, int groups_per_tile) {
    // col: .x = source byte offset of the left tap within a row (-1: border), .y = a0 | a1 << 16
    __shared__ __attribute__((aligned(16))) int2 col[LB_TILE_GROUPS * 4];
    __shared__ int4 row[LB_ROWS];                // .x = y0 (-1: border row), .y = y1, .z = b0, .w = b1
    const Frame f = table[blockIdx.y];           // uniform address: scalar loads
    const gbytes src = (gbytes)f.src;
    const int tile = (int)(blockIdx.x % (unsigned)tiles_x), rblk = (int)(blockIdx.x / (unsigned)tiles_x);
    const int groups = width >> 2;
    const int g_begin = tile * groups_per_tile, g_end = min(groups, g_begin + groups_per_tile);
    const int n_groups = g_end - g_begin;
    const int x_begin = g_begin * 4, n_cols = n_groups * 4;
    const int row_begin = rblk * LB_ROWS, n_rows = min(LB_ROWS, height - row_begin);

    // OpenCV: inv_scale = dsize / ssize (double), scale = 1 / inv_scale
    const double scale_x = 1.0 / ((double)f.new_w / (double)f.w), scale_y = 1.0 / ((double)f.new_h / (double)f.h);
    for (int i = threadIdx.x; i < n_cols; i += LB_THREADS) {
        const int dx = x_begin + i - f.pad_left;
        int2 e = make_int2(-1, 0);
        if (dx >= 0 && dx < f.new_w) {
            int sx;
            float fx;
            axis_coef(dx, scale_x, sx, fx);
            if (sx < 0) { fx = 0.f; sx = 0; }
            if (sx >= f.w - 1) { fx = 0.f; sx = f.w - 1; }
            const int a0 = (short)__float2int_rn((1.f - fx) * 2048.f), a1 = (short)__float2int_rn(fx * 2048.f);
            e = make_int2(sx * C, (a0 & 0xffff) | (a1 << 16));
        }
        col[i] = e;
    }
    if ((int)threadIdx.x < n_rows) {
        const int dy = row_begin + (int)threadIdx.x - f.pad_top;
        int4 e = make_int4(-1, 0, 0, 0);
        if (dy >= 0 && dy < f.new_h) {
            int sy;
            float fy;
            axis_coef(dy, scale_y, sy, fy);       // fy is not clamped: the two source rows are clipped to the image instead
            e.x = min(max(sy, 0), f.h - 1);
            e.y = min(max(sy + 1, 0), f.h - 1);
            e.z = (short)__float2int_rn((1.f - fy) * 2048.f);
            e.w = (short)__float2int_rn(fy * 2048.f);
        }
        row[threadIdx.x] = e;
    }
    __syncthreads();

    const int row_bytes = f.w * C;               // bytes of a source row that belong to the frame (row_stride may be larger)
    const bool wide = row_bytes >= 8;
    unsigned char* const canvas = out + (size_t)blockIdx.y * height * width * C;
    const int items = n_rows * n_groups;
    for (int i = threadIdx.x; i < items; i += LB_THREADS) {
        const int r = i / n_groups, g = i - r * n_groups;
        const int4 rc = row[r];
        unsigned px[4];                          // pixel p's C channel bytes, channel c at bits 8c
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = fill;
        if (rc.x >= 0) {
            const gbytes r0 = src + (size_t)rc.x * f.row_stride;
            const gbytes r1 = src + (size_t)rc.y * f.row_stride;
            const int4 c01 = reinterpret_cast<const int4*>(col)[g * 2], c23 = reinterpret_cast<const int4*>(col)[g * 2 + 1];
            const int2 c4[4] = {make_int2(c01.x, c01.y), make_int2(c01.z, c01.w), make_int2(c23.x, c23.y), make_int2(c23.z, c23.w)};
            // all eight loads of the group are issued before the first is used; a border pixel reads its row's first bytes and drops them
            unsigned long long t0[4], t1[4];     // bytes 0..C-1: left tap, C..2C-1: right tap
            if (wide) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int x0 = max(c4[p].x, 0), o = min(x0, row_bytes - 8);
                    t0[p] = *(gwords)(r0 + o);
                    t1[p] = *(gwords)(r1 + o);
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int x0 = max(c4[p].x, 0), sh = (x0 - min(x0, row_bytes - 8)) * 8;
                    t0[p] >>= sh;
                    t1[p] >>= sh;
                }
            } else {
                for (int p = 0; p < 4; ++p) {
                    const int x0 = max(c4[p].x, 0);
                    t0[p] = t1[p] = 0;
                    for (int b = 0; b < 2 * C && x0 + b < row_bytes; ++b) {
                        t0[p] |= (unsigned long long)r0[x0 + b] << (8 * b);
                        t1[p] |= (unsigned long long)r1[x0 + b] << (8 * b);
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a0 = (short)(c4[p].y & 0xffff), a1 = c4[p].y >> 16;
                // at the last column the right tap's bytes are zeros shifted in: its weight a1 is 0 there
                unsigned v4 = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int d0 = (int)((t0[p] >> (8 * c)) & 255u) * a0 + (int)((t0[p] >> (8 * (c + C))) & 255u) * a1;
                    const int d1 = (int)((t1[p] >> (8 * c)) & 255u) * a0 + (int)((t1[p] >> (8 * (c + C))) & 255u) * a1;
                    const int v = (((rc.z * (d0 >> 4)) >> 16) + ((rc.w * (d1 >> 4)) >> 16) + 2) >> 2;
                    v4 |= (unsigned)min(max(v, 0), 255) << (8 * c);
                }
                if (c4[p].x >= 0) px[p] = v4;
            }
        }
        unsigned* dst = reinterpret_cast<unsigned*>(canvas + ((size_t)(row_begin + r) * width + (size_t)(g_begin + g) * 4) * C);
#pragma unroll
        for (int k = 0; k < C; ++k) {            // word k of the group: byte 4k + b = channel (4k + b) % C of pixel (4k + b) / C
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= ((px[(4 * k + b) / C] >> (8 * ((4 * k + b) % C))) & 255u) << (8 * b);
            dst[k] = v;
        }
    }
}

// boxes [N, k, 4] (x1 y1 x2 y2) in canvas pixels -> the frame's own pixels, in place; one thread per box (one 16-byte load and store)
__global__ __launch_bounds__(256) void unletterbox_kernel(float4* __restrict__ boxes, const Frame* __restrict__ table, int N, int k, int clip) {
    const long total = (long)N * k;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const Frame& f = table[t / k];
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

template <int C>
static int launch(const void* table, uint8_t* out, int N, int height, int width, unsigned fill, hipStream_t stream) {
    const int groups = width / 4;
    const int tiles_x = (groups + LB_TILE_GROUPS - 1) / LB_TILE_GROUPS;
    const int groups_per_tile = (groups + tiles_x - 1) / tiles_x;           // equal tiles: 1088 columns = 2 x 136 groups, not 256 + 16
    const int row_blocks = (height + LB_ROWS - 1) / LB_ROWS;
    hipLaunchKernelGGL(letterbox_kernel<C>, dim3((unsigned)(tiles_x * row_blocks), (unsigned)N), dim3(LB_THREADS), 0, stream,
                       static_cast<const Frame*>(table), out, height, width, fill, tiles_x, groups_per_tile);
    return cnl::check_launch("letterbox_kernel");
}

}  // namespace cnl_letterbox

extern "C" int cnl_letterbox_bilinear_u8(const void* table, uint8_t* out, int32_t N, int32_t height, int32_t width, int32_t C,
                                         uint32_t fill_rgba, void* stream) {
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "cnl_letterbox_bilinear_u8: N = %d outside 0..65535", N);
    CNL_REQUIRE(C >= 1 && C <= 4, CNL_E_BAD_ARG, "cnl_letterbox_bilinear_u8: C = %d outside 1..4", C);
    CNL_REQUIRE(height > 0 && width > 0 && height % 32 == 0 && width % 32 == 0, CNL_E_BAD_ARG,
                "cnl_letterbox_bilinear_u8: canvas %d x %d is not a positive multiple of 32", height, width);
    CNL_REQUIRE((long)height * width * C <= 0x7fffffffL, CNL_E_BAD_ARG, "cnl_letterbox_bilinear_u8: the canvas of one frame exceeds 2 GiB");
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(table && out, CNL_E_BAD_ARG, "cnl_letterbox_bilinear_u8: null pointer");
    CNL_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)out & 3) == 0, CNL_E_BAD_ARG,
                "cnl_letterbox_bilinear_u8: table must be 8-byte and out 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: return cnl_letterbox::launch<1>(table, out, N, height, width, fill_rgba, s);
        case 2: return cnl_letterbox::launch<2>(table, out, N, height, width, fill_rgba, s);
        case 3: return cnl_letterbox::launch<3>(table, out, N, height, width, fill_rgba, s);
        default: return cnl_letterbox::launch<4>(table, out, N, height, width, fill_rgba, s);
    }
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
                       reinterpret_cast<float4*>(boxes), static_cast<const cnl_letterbox::Frame*>(table), N, k, clip);
    return cnl::check_launch("unletterbox_kernel");
}
