// letterbox_yuv.hip — letterbox.hip's canvas straight from YUV 4:2:0 video surfaces (NV12 / I420): the colour conversion happens on the
// resize's taps in registers, so the RGB frame between the decoder and the network is never written.
//
//   letterbox_yuv420_kernel   N frames (or windows of frames: tiles), each with its own size, planes and pitches, -> one
//                             [N, height, width, 3] RGB canvas, bit for bit letterbox_kernel<3> on the frames converted by the integer
//                             rule of include/centernet_gfx950.h (OpenCV's cvtColor arithmetic, nearest chroma).
//
// The decomposition is letterbox_kernel's and so are the axis tables (restated here, not shared: letterbox.hip stays as it is): the
// canvas is tiled, never the frame; grid.y = record, grid.x = (block of LB_ROWS canvas rows) x (column tile of <= 1024 columns); the
// per-column and per-row terms are computed once per workgroup into LDS; a thread owns 4 canvas pixels = three whole 32-bit words;
// every canvas byte is written exactly once.  What differs is the tap: a canvas pixel reads 2 x 2 Y bytes and the chroma sample of
// each (one 2-byte load per tap for NV12's interleaved UV, two byte loads for I420), converts the four source pixels to RGB and then
// applies the 11-bit fixed-point interpolation of letterbox_kernel unchanged.  All loads of a thread's group are issued before the
// first is used.  A frame's bytes are read (2 rows of Y and 1-2 rows of chroma per canvas row) at 1.5 bytes per source pixel instead
// of 3.  Measured rate: DESIGN.md §15.
#include <algorithm>
#include <cstdlib>
#include "cnl_common.h"

#pragma clang fp contract(off)   // OpenCV rounds (dx + 0.5) * scale and the subtraction separately

namespace cnl_letterbox_yuv {

constexpr int LB_THREADS = 256;
constexpr int LB_ROWS = 8;           // canvas rows per workgroup
constexpr int LB_TILE_GROUPS = 256;  // 4-pixel groups per column tile (1024 canvas columns)

typedef cnl_yuv420_frame Frame;      // include/centernet_gfx950.h (72 bytes)
struct Coef {
    int y_off, cy, cvr, cvg, cug, cub;
};
typedef unsigned short u16_unaligned __attribute__((aligned(1)));
// the planes' pointers come out of the table, so the compiler cannot tell their address space: name it (global_load, not flat_load)
typedef const __attribute__((address_space(1))) unsigned char* gbytes;
typedef const __attribute__((address_space(1))) u16_unaligned* gpairs;

// letterbox_kernel's (= resize_bilinear_u8_kernel's) coefficient rule for one axis position
__device__ __forceinline__ void axis_coef(int d, double scale, int& s, float& f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}

__device__ __forceinline__ unsigned sat8(int v) { return (unsigned)min(max(v, 0), 255); }

// one source pixel -> R | G << 8 | B << 16
__device__ __forceinline__ unsigned yuv_to_rgb(int Y, int U, int V, const Coef& k) {
    const int yy = max(Y - k.y_off, 0) * k.cy + (1 << 19), u = U - 128, v = V - 128;
    return sat8((yy + k.cvr * v) >> 20) | (sat8((yy + k.cvg * v + k.cug * u) >> 20) << 8) | (sat8((yy + k.cub * u) >> 20) << 16);
}

__global__ __launch_bounds__(LB_THREADS) void letterbox_yuv420_kernel(const Frame* __restrict__ table, unsigned char* __restrict__ out,
                                                                      int height, int width, Coef k, unsigned fill, int tiles_x,
                                                                      int groups_per_tile) {
    // col: .x = window column of the left tap (-1: border), .y = a0 | a1 << 16
    __shared__ __attribute__((aligned(16))) int2 col[LB_TILE_GROUPS * 4];
    __shared__ int4 row[LB_ROWS];                // .x = y0 (-1: border row), .y = y1, .z = b0, .w = b1
    const Frame f = table[blockIdx.y];           // uniform address: scalar loads
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
            e = make_int2(sx, (a0 & 0xffff) | (a1 << 16));
        }
        col[i] = e;
    }
    if ((int)threadIdx.x < n_rows) {
        const int dy = row_begin + (int)threadIdx.x - f.pad_top;
        int4 e = make_int4(-1, 0, 0, 0);
        if (dy >= 0 && dy < f.new_h) {
            int sy;
            float fy;
            axis_coef(dy, scale_y, sy, fy);       // fy is not clamped: the two source rows are clipped to the window instead
            e.x = min(max(sy, 0), f.h - 1);
            e.y = min(max(sy + 1, 0), f.h - 1);
            e.z = (short)__float2int_rn((1.f - fy) * 2048.f);
            e.w = (short)__float2int_rn(fy * 2048.f);
        }
        row[threadIdx.x] = e;
    }
    __syncthreads();

    const gbytes yp = (gbytes)f.y, up = (gbytes)f.u, vp = (gbytes)f.v;
    const bool interleaved = f.c_step == 2 && f.v == (const void*)((const unsigned char*)f.u + 1);      // NV12: U and V in one 2-byte load
    unsigned char* const canvas = out + (size_t)blockIdx.y * height * width * 3;
    const int items = n_rows * n_groups;
    for (int i = threadIdx.x; i < items; i += LB_THREADS) {
        const int r = i / n_groups, g = i - r * n_groups;
        const int4 rc = row[r];
        unsigned px[4];                          // pixel p's bytes: R at bits 0, G at 8, B at 16
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = fill;
        if (rc.x >= 0) {
            const int fy0 = f.y0 + rc.x, fy1 = f.y0 + rc.y;                 // the two source rows, in frame coordinates
            const gbytes y0r = yp + (size_t)fy0 * f.y_pitch, y1r = yp + (size_t)fy1 * f.y_pitch;
            const size_t c0r = (size_t)(fy0 >> 1) * f.c_pitch, c1r = (size_t)(fy1 >> 1) * f.c_pitch;
            const int4 c01 = reinterpret_cast<const int4*>(col)[g * 2], c23 = reinterpret_cast<const int4*>(col)[g * 2 + 1];
            const int2 c4[4] = {make_int2(c01.x, c01.y), make_int2(c01.z, c01.w), make_int2(c23.x, c23.y), make_int2(c23.z, c23.w)};
            // tap t of pixel p: t = 0 (row 0, left), 1 (row 0, right), 2 (row 1, left), 3 (row 1, right).  All loads are issued before
            // the first is used; a border pixel reads its row's first column and drops it.  The right tap of the window's last
            // column is the left tap again: its weight a1 is 0 there.
            int Y[4][4], UV[4][4];               // UV = U | V << 8
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int sx = max(c4[p].x, 0);
                const int xl = f.x0 + sx, xr = f.x0 + min(sx + 1, f.w - 1);
                const int cl = (xl >> 1) * f.c_step, cr = (xr >> 1) * f.c_step;
                Y[p][0] = y0r[xl];
                Y[p][1] = y0r[xr];
                Y[p][2] = y1r[xl];
                Y[p][3] = y1r[xr];
                if (interleaved) {
                    UV[p][0] = *(gpairs)(up + c0r + cl);
                    UV[p][1] = *(gpairs)(up + c0r + cr);
                    UV[p][2] = *(gpairs)(up + c1r + cl);
                    UV[p][3] = *(gpairs)(up + c1r + cr);
                } else {
                    UV[p][0] = up[c0r + cl] | (vp[c0r + cl] << 8);
                    UV[p][1] = up[c0r + cr] | (vp[c0r + cr] << 8);
                    UV[p][2] = up[c1r + cl] | (vp[c1r + cl] << 8);
                    UV[p][3] = up[c1r + cr] | (vp[c1r + cr] << 8);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a0 = (short)(c4[p].y & 0xffff), a1 = c4[p].y >> 16;
                unsigned t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = yuv_to_rgb(Y[p][q], UV[p][q] & 255, UV[p][q] >> 8, k);
                unsigned v4 = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {    // letterbox_kernel's interpolation, to the letter
                    const int d0 = (int)((t[0] >> (8 * c)) & 255u) * a0 + (int)((t[1] >> (8 * c)) & 255u) * a1;
                    const int d1 = (int)((t[2] >> (8 * c)) & 255u) * a0 + (int)((t[3] >> (8 * c)) & 255u) * a1;
                    const int v = (((rc.z * (d0 >> 4)) >> 16) + ((rc.w * (d1 >> 4)) >> 16) + 2) >> 2;
                    v4 |= (unsigned)min(max(v, 0), 255) << (8 * c);
                }
                if (c4[p].x >= 0) px[p] = v4;
            }
        }
        unsigned* dst = reinterpret_cast<unsigned*>(canvas + ((size_t)(row_begin + r) * width + (size_t)(g_begin + g) * 4) * 3);
#pragma unroll
        for (int w = 0; w < 3; ++w) {            // word w of the group: byte 4w + b = channel (4w + b) % 3 of pixel (4w + b) / 3
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= ((px[(4 * w + b) / 3] >> (8 * ((4 * w + b) % 3))) & 255u) << (8 * b);
            dst[w] = v;
        }
    }
}

}  // namespace cnl_letterbox_yuv

extern "C" int cnl_letterbox_yuv420_u8(const void* table, uint8_t* out, int32_t N, int32_t height, int32_t width, const int32_t* coef,
                                       uint32_t fill_rgba, void* stream) {
    using namespace cnl_letterbox_yuv;
    static_assert(sizeof(Frame) == 72, "cnl_yuv420_frame is 72 bytes");
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "cnl_letterbox_yuv420_u8: N = %d outside 0..65535", N);
    CNL_REQUIRE(height > 0 && width > 0 && height % 32 == 0 && width % 32 == 0, CNL_E_BAD_ARG,
                "cnl_letterbox_yuv420_u8: canvas %d x %d is not a positive multiple of 32", height, width);
    CNL_REQUIRE((long)height * width * 3 <= 0x7fffffffL, CNL_E_BAD_ARG, "cnl_letterbox_yuv420_u8: the canvas of one frame exceeds 2 GiB");
    CNL_REQUIRE(coef, CNL_E_BAD_ARG, "cnl_letterbox_yuv420_u8: null coefficients");
    const Coef k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    const long chroma = std::max(std::max(std::labs((long)k.cvr), std::labs((long)k.cvg) + std::labs((long)k.cug)), std::labs((long)k.cub));
    CNL_REQUIRE(k.y_off >= 0 && k.y_off <= 255 && k.cy >= 0 && 255L * k.cy + (1L << 19) + 128L * chroma < (1L << 31), CNL_E_UNSUPPORTED,
                "cnl_letterbox_yuv420_u8: coefficients {%d, %d, %d, %d, %d, %d} can overflow 32-bit arithmetic", k.y_off, k.cy, k.cvr, k.cvg,
                k.cug, k.cub);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(table && out, CNL_E_BAD_ARG, "cnl_letterbox_yuv420_u8: null pointer");
    CNL_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)out & 3) == 0, CNL_E_BAD_ARG,
                "cnl_letterbox_yuv420_u8: table must be 8-byte and out 4-byte aligned");
    const int groups = width / 4;
    const int tiles_x = (groups + LB_TILE_GROUPS - 1) / LB_TILE_GROUPS;
    const int groups_per_tile = (groups + tiles_x - 1) / tiles_x;           // equal tiles, as letterbox.hip's launch
    const int row_blocks = (height + LB_ROWS - 1) / LB_ROWS;
    hipLaunchKernelGGL(letterbox_yuv420_kernel, dim3((unsigned)(tiles_x * row_blocks), (unsigned)N), dim3(LB_THREADS), 0,
                       (hipStream_t)stream, static_cast<const Frame*>(table), out, height, width, k, fill_rgba, tiles_x, groups_per_tile);
    return cnl::check_launch("letterbox_yuv420_kernel");
}
