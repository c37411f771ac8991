// letterbox_sampling.h — the ONE copy of the cv2 INTER_LINEAR window-to-rectangle sampling rule (resize_bilinear_u8_kernel's 8-bit
// fixed-point arithmetic, bit for bit) that letterbox.hip (letterbox_kernel: the letterbox, tile, crop and YUV entries) and augment.hip
// (augment_kernel: several placements per canvas, mirrored, colour-twisted) both run:
//   axis_coef        source position and fraction of one destination position on one axis
//   column_entry     what a kernel's column table keeps for one destination column (left tap, the two 11-bit weights)
//   row_entry        what its row table keeps for one destination row (the two source rows clipped to the window, the two weights)
//   PackedSource<C>  a window of packed C-channel bytes and its unaligned 8-byte tap loads
//   sample_group     the four pixels of a thread's group from their taps: the >> 4 ... >> 16 ... + 2 >> 2 accumulation
//   store_group      the group's 4 * C bytes as C whole 32-bit words
// A kernel builds its tables in LDS once per workgroup and calls sample_group per 4-pixel group; nothing here is recomputed per pixel.
#pragma once
#include "cnl_common.h"

#pragma clang fp contract(off)   // OpenCV rounds (dx + 0.5) * scale and the subtraction separately

namespace cnl_letterbox {

constexpr int LB_THREADS = 256;
constexpr int LB_ROWS = 8;           // canvas rows per workgroup (the two letterbox entries, the augment entry)
constexpr int LB_TILE_GROUPS = 256;  // 4-pixel groups per column tile (1024 canvas columns)

typedef unsigned short u16_unaligned __attribute__((aligned(1)));
typedef unsigned long long u64_unaligned __attribute__((aligned(1)));
// the frames' pointers come out of the table, so the compiler cannot tell their address space: name it (global_load, not flat_load)
typedef const __attribute__((address_space(1))) unsigned char* gbytes;
typedef const __attribute__((address_space(1))) u16_unaligned* gpairs;
typedef const __attribute__((address_space(1))) u64_unaligned* gwords;

// resize_bilinear_u8_kernel's coefficient rule for one axis position
__device__ __forceinline__ void axis_coef(int d, double scale, int& s, float& f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}

// OpenCV: inv_scale = dsize / ssize (double), scale = 1 / inv_scale
__device__ __forceinline__ double axis_scale(int dsize, int ssize) { return 1.0 / ((double)dsize / (double)ssize); }

// destination column dx (0 <= dx < new_w) of a window w columns wide: .x = Source::column of the left tap's source column, .y = a0 | a1 << 16
template <class Source>
__device__ __forceinline__ int2 column_entry(int dx, double scale_x, int w) {
    int sx;
    float fx;
    axis_coef(dx, scale_x, sx, fx);
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= w - 1) { fx = 0.f; sx = w - 1; }
    const int a0 = (short)__float2int_rn((1.f - fx) * 2048.f), a1 = (short)__float2int_rn(fx * 2048.f);
    return make_int2(Source::column(sx), (a0 & 0xffff) | (a1 << 16));
}

// destination row dy (0 <= dy < new_h) of a window h rows high: .x = y0, .y = y1, .z = b0, .w = b1
__device__ __forceinline__ int4 row_entry(int dy, double scale_y, int h) {
    int sy;
    float fy;
    axis_coef(dy, scale_y, sy, fy);               // fy is not clamped: the two source rows are clipped to the frame (window) instead
    int4 e;
    e.x = min(max(sy, 0), h - 1);
    e.y = min(max(sy + 1, 0), h - 1);
    e.z = (short)__float2int_rn((1.f - fy) * 2048.f);
    e.w = (short)__float2int_rn(fy * 2048.f);
    return e;
}

// packed C-channel bytes (cnl_letterbox_frame, 40 bytes); the column table keeps the byte offset of the left tap within a row
template <int CH>
struct PackedSource {
    static constexpr int C = CH;
    typedef cnl_letterbox_frame Frame;
    struct Params {};
    struct Taps {
        unsigned long long t0[4], t1[4];         // per pixel, upper / lower source row; bytes 0..C-1: left tap, C..2C-1: right tap
    };
    const Frame& f;
    const gbytes src;
    const int row_bytes;                         // bytes of a source row that belong to the frame (row_stride may be larger)
    const bool wide;

    __device__ __forceinline__ PackedSource(const Frame& f, const Params&) : f(f), src((gbytes)f.src), row_bytes(f.w * C), wide(row_bytes >= 8) {}
    static __device__ __forceinline__ int column(int sx) { return sx * C; }

    // a border pixel (c4[p].x < 0) reads its row's first bytes; the caller drops them
    __device__ __forceinline__ void load(int y0, int y1, const int2 (&c4)[4], Taps& t) const {
        const gbytes r0 = src + (size_t)y0 * f.row_stride;
        const gbytes r1 = src + (size_t)y1 * f.row_stride;
        if (wide) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int x0 = max(c4[p].x, 0), o = min(x0, row_bytes - 8);
                t.t0[p] = *(gwords)(r0 + o);
                t.t1[p] = *(gwords)(r1 + o);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int x0 = max(c4[p].x, 0), sh = (x0 - min(x0, row_bytes - 8)) * 8;
                t.t0[p] >>= sh;
                t.t1[p] >>= sh;
            }
        } else {
            for (int p = 0; p < 4; ++p) {
                const int x0 = max(c4[p].x, 0);
                t.t0[p] = t.t1[p] = 0;
                for (int b = 0; b < 2 * C && x0 + b < row_bytes; ++b) {
                    t.t0[p] |= (unsigned long long)r0[x0 + b] << (8 * b);
                    t.t1[p] |= (unsigned long long)r1[x0 + b] << (8 * b);
                }
            }
        }
    }
    // at the last column the right tap's bytes are zeros shifted in: its weight a1 is 0 there
    __device__ __forceinline__ void taps(const Taps& t, int p, unsigned (&v)[4]) const {
        v[0] = (unsigned)t.t0[p];
        v[1] = (unsigned)(t.t0[p] >> (8 * C));
        v[2] = (unsigned)t.t1[p];
        v[3] = (unsigned)(t.t1[p] >> (8 * C));
    }
};

// the four pixels of one group on the table row rc (row_entry) and the table columns c4 (column_entry; .x < 0: a border pixel, whose px[p]
// is left as it was): px[p] = pixel p's C channel bytes, channel c at bits 8c
template <class Source>
__device__ __forceinline__ void sample_group(const Source& source, const int4& rc, const int2 (&c4)[4], unsigned (&px)[4]) {
    constexpr int C = Source::C;
    typename Source::Taps loaded;
    source.load(rc.x, rc.y, c4, loaded);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int a0 = (short)(c4[p].y & 0xffff), a1 = c4[p].y >> 16;
        unsigned t[4];
        source.taps(loaded, p, t);
        unsigned v4 = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int d0 = (int)((t[0] >> (8 * c)) & 255u) * a0 + (int)((t[1] >> (8 * c)) & 255u) * a1;
            const int d1 = (int)((t[2] >> (8 * c)) & 255u) * a0 + (int)((t[3] >> (8 * c)) & 255u) * a1;
            const int v = (((rc.z * (d0 >> 4)) >> 16) + ((rc.w * (d1 >> 4)) >> 16) + 2) >> 2;
            v4 |= (unsigned)min(max(v, 0), 255) << (8 * c);
        }
        if (c4[p].x >= 0) px[p] = v4;
    }
}

// word k of the group: byte 4k + b = channel (4k + b) % C of pixel (4k + b) / C
template <int C>
__device__ __forceinline__ void store_group(unsigned* dst, const unsigned (&px)[4]) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
        unsigned v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= ((px[(4 * k + b) / C] >> (8 * ((4 * k + b) % C))) & 255u) << (8 * b);
        dst[k] = v;
    }
}

}  // namespace cnl_letterbox
