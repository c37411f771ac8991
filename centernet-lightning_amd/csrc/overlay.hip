// overlay.hip — cnl_draw_boxes_u8: detections drawn onto the frames they were found in (packed RGB / RGBA bytes or the planes of
// NV12 / I420 surfaces, mixed sizes, painted in place): box outlines, optional half-transparent fills and decimal number tags.
// The output side of the frame pipeline, the twin of cnl_crop_boxes_u8 (letterbox.hip); the rule is stated in
// include/centernet_gfx950.h and restated in numpy by tests/overlay_ref.py.  Everything is integer once the corners are rounded.
//
//   overlay_records_kernel<Frame>  one thread per slot (n, j): box + gates + label + number -> one 64-byte integer SlotRecord (the
//                                  influence rectangle clipped to the frame, the corners, the tag, the colour, the digits).  All
//                                  float work happens here, once.
//   overlay_paint_kernel<Format>   grid.x = 64 x 16-sample tiles of the LARGEST frame, grid.y = frame, grid.z = plane (Y / UV or
//                                  U / V of a YUV frame).  A workgroup whose tile lies outside its plane returns at once; otherwise
//                                  it scans the frame's k records from j = k - 1 downwards, 256 per chunk (one 16-byte load per
//                                  thread: the influence rectangle), and keeps those that touch its tile, IN ORDER, in an LDS list:
//                                  ballot + popcount prefix inside a wave, the four wave totals through LDS.  Not an atomic append:
//                                  the order is the result.  A workgroup that no record touches has read k rectangles and no pixel:
//                                  the cost follows the painted area, not the frame area.
//                                  A thread owns 4 neighbouring samples of one row (every byte has one owner), loads them when the
//                                  first non-empty list arrives, carries them in registers through every list, and stores them at
//                                  the end if a layer touched them.  Where the plane's base and pitch are 4-byte aligned a full
//                                  group is whole dwords (3 at C = 3, 4 at C = 4, 1 for Y, 2 for interleaved UV); otherwise, and for
//                                  the last partial group of a row, single bytes (a frame sliced out of an [N, h, w, 3] tensor with
//                                  odd h * w is not aligned).  Bytes beyond a row's visible samples are never read or written.
//                                  The list entries are read by all lanes at one address (LDS broadcast).
// A chroma sample (cy, cx) is painted as the pixel (2 cy, 2 cx): the same body with the coordinates shifted.
#include <algorithm>
#include "cnl_common.h"

#pragma clang fp contract(off)   // the corner rule is single fp32 operations

namespace cnl_overlay {

constexpr int OV_THREADS = 256;
constexpr int OV_TILE_W = 64, OV_TILE_H = 16;    // samples of a plane per workgroup: 256 threads x 4 samples of one row
constexpr int OV_CHUNK = OV_THREADS;             // records looked at per scan step, one per thread
constexpr int OV_DEAD = 0x7fffffff;              // rx0 = ry0 of a slot that paints nothing (rx1 = ry1 = -1): no tile, no pixel passes

typedef __attribute__((address_space(1))) unsigned char* gbytes;
typedef __attribute__((address_space(1))) unsigned* gwords;
static_assert(sizeof(cnl_letterbox_frame) == 40 && sizeof(cnl_yuv420_frame) == 72, "the frame records of include/centernet_gfx950.h");

struct SlotRecord {                              // 64 bytes = four 16-byte words
    int rx0, ry0, rx1, ry1;                      // everything the slot paints, clipped to the frame, inclusive
    int x1, y1, x2, y2;                          // the rounded corners
    int tag_x, tag_y, tag_w, digits;             // the tag's left, top and width in pixels (width 0: no tag), its digit count
    unsigned colour, digits_lo, digits_hi, reserved;     // digit q (0 = most significant) at bits 4q of digits_hi:digits_lo
};
static_assert(sizeof(SlotRecord) == 64, "SlotRecord is 64 bytes");

struct Style {
    int k, P, t, o, i, alpha, scale;
    float threshold;
};

// five bits per row, rows top to bottom at bits 5 * row, the most significant of the five is the left column
constexpr unsigned long long glyph(unsigned r0, unsigned r1, unsigned r2, unsigned r3, unsigned r4, unsigned r5, unsigned r6) {
    return (unsigned long long)r0 | (unsigned long long)r1 << 5 | (unsigned long long)r2 << 10 | (unsigned long long)r3 << 15 |
           (unsigned long long)r4 << 20 | (unsigned long long)r5 << 25 | (unsigned long long)r6 << 30;
}
__constant__ unsigned long long GLYPHS[10] = {
    glyph(0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110), glyph(0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    glyph(0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111), glyph(0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110),
    glyph(0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010), glyph(0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110),
    glyph(0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110), glyph(0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000),
    glyph(0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110), glyph(0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100),
};

// rintf, then the two clamps in float, then the conversion (a NaN becomes -32768; its slot is dead anyway)
__device__ __forceinline__ int corner(float x) {
    float v = rintf(x);
    v = v > -32768.f ? v : -32768.f;
    v = v < 32767.f ? v : 32767.f;
    return (int)v;
}

// one thread per slot (n, j) of boxes [N, k, 4]
template <class Frame>
__global__ __launch_bounds__(256) void overlay_records_kernel(const Frame* __restrict__ frames, const float4* __restrict__ boxes,
                                                              const long long* __restrict__ labels, const int* __restrict__ numbers,
                                                              const float* __restrict__ scores, const int* __restrict__ count,
                                                              const unsigned* __restrict__ palette, SlotRecord* __restrict__ records, long total,
                                                              Style q) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int n = (int)(t / q.k), j = (int)(t - (long)n * q.k);
    const int W = frames[n].w, H = frames[n].h;
    const float4 b = boxes[t];
    const bool live = (!count || j < count[n]) && (!scores || scores[t] >= q.threshold) && __builtin_isfinite(b.x) &&
                      __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && __builtin_isfinite(b.w);
    SlotRecord r = {};
    r.rx0 = r.ry0 = OV_DEAD;
    r.rx1 = r.ry1 = -1;
    r.x1 = corner(b.x);
    r.y1 = corner(b.y);
    r.x2 = corner(b.z);
    r.y2 = corner(b.w);
    if (live && r.x2 >= r.x1 && r.y2 >= r.y1) {
        long long l = labels ? labels[t] % q.P : 0;
        if (l < 0) l += q.P;
        r.colour = palette[l];
        int ux0 = r.x1 - q.o, uy0 = r.y1 - q.o, ux1 = r.x2 + q.o, uy1 = r.y2 + q.o;
        const int m = numbers ? numbers[t] : -1;
        if (q.scale > 0 && m >= 0) {
            unsigned v = (unsigned)m;
            int d = 1;
            for (unsigned p = 10; d < 10 && v >= p; p *= 10) ++d;
            unsigned long long dg = 0;
            for (int e = d - 1; e >= 0; --e) {
                dg |= (unsigned long long)(v % 10u) << (4 * e);
                v /= 10u;
            }
            r.digits = d;
            r.digits_lo = (unsigned)dg;
            r.digits_hi = (unsigned)(dg >> 32);
            r.tag_w = (6 * d + 1) * q.scale;
            r.tag_x = ux0;
            r.tag_y = uy0 - 9 * q.scale;
            if (r.tag_y < 0) r.tag_y = uy0;
            ux1 = max(ux1, r.tag_x + r.tag_w - 1);
            uy0 = min(uy0, r.tag_y);
            uy1 = max(uy1, r.tag_y + 9 * q.scale - 1);
        }
        ux0 = max(ux0, 0);
        uy0 = max(uy0, 0);
        ux1 = min(ux1, W - 1);
        uy1 = min(uy1, H - 1);
        if (ux0 <= ux1 && uy0 <= uy1) {          // (a live box wholly outside the frame paints nothing)
            r.rx0 = ux0;
            r.ry0 = uy0;
            r.rx1 = ux1;
            r.ry1 = uy1;
        }
    }
    records[t] = r;
}

// one plane of one frame as the painter sees it
struct Plane {
    unsigned char* base;
    int pitch, step;                             // bytes from one row / one sample to the next
    int w, h;                                    // samples
    int sub;                                     // sample (sy, sx) is the pixel (sy << sub, sx << sub)
    int coff;                                    // channel c is painted with byte coff + c of a colour
};

struct PaintShared {
    int4 list[OV_CHUNK * 4];                     // the records that touch this tile, in painting order
    int wave_n[2][OV_THREADS / 64];              // per scan step (two alternate): how many each wave kept
};

// STEP: bytes per sample where the dword path may be taken (0: pl.step, bytes only); NC: channels painted (<= STEP)
template <int STEP, int NC>
__device__ __forceinline__ void paint(const Plane& pl, const SlotRecord* __restrict__ recs, const Style& q, unsigned text_colour, int tile_x,
                                      int tile_y, PaintShared& sh) {
    static_assert(NC >= 1 && NC <= 3 && (STEP == 0 || (STEP >= NC && STEP <= 4)), "1..3 painted channels in samples of up to 4 bytes");
    const int sx0 = tile_x * OV_TILE_W, sy0 = tile_y * OV_TILE_H;
    if (sx0 >= pl.w || sy0 >= pl.h) return;      // (uniform) the tile lies outside this plane
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the tile in pixels, inclusive
    const int px0 = sx0 << pl.sub, px1 = min(sx0 + OV_TILE_W - 1, pl.w - 1) << pl.sub;
    const int py0 = sy0 << pl.sub, py1 = min(sy0 + OV_TILE_H - 1, pl.h - 1) << pl.sub;
    // this thread's 4 samples
    const int sx = sx0 + (tid % (OV_TILE_W / 4)) * 4, sy = sy0 + tid / (OV_TILE_W / 4);
    const int n_valid = sy < pl.h ? min(max(pl.w - sx, 0), 4) : 0;
    const int y = sy << pl.sub, xf = sx << pl.sub, xl = (sx + max(n_valid, 1) - 1) << pl.sub;
    const int step = STEP ? STEP : pl.step;
    const bool wide = STEP != 0 && n_valid == 4 && (((size_t)pl.base | (size_t)pl.pitch) & 3) == 0;
    const gbytes row = (gbytes)pl.base + (size_t)sy * pl.pitch + (size_t)sx * step;

    constexpr int WORDS = STEP ? STEP : 1;
    unsigned words[WORDS] = {};                     // the dword path's bytes as loaded: what is not painted (channel 3) goes back as it came
    int px[4][NC];
    bool loaded = false;
    unsigned dirty = 0;                          // bit p: sample p was painted

    for (int c0 = 0, it = 0; c0 < q.k; c0 += OV_CHUNK, ++it) {
        const int j = q.k - 1 - (c0 + tid);
        bool hit = false;
        if (j >= 0) {
            const int4 a = reinterpret_cast<const int4*>(recs + j)[0];
            hit = a.x <= px1 && a.z >= px0 && a.y <= py1 && a.w >= py0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) sh.wave_n[it & 1][wave] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < OV_THREADS / 64; ++w) {
            const int c = sh.wave_n[it & 1][w];
            base += w < wave ? c : 0;
            total += c;
        }
        if (total == 0) continue;                // (uniform) nothing of this chunk touches the tile; the other wave_n serves the next step
        if (hit) {
            const int at = base + __popcll(m & ((1ull << lane) - 1ull));
            const int4* src = reinterpret_cast<const int4*>(recs + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) sh.list[at * 4 + e] = src[e];
        }
        __syncthreads();
        if (!loaded) {
            loaded = true;
            if (wide) {
#pragma unroll
                for (int e = 0; e < WORDS; ++e) words[e] = ((gwords)row)[e];
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < NC; ++c) px[p][c] = (int)((words[(p * WORDS + c) / 4] >> (8 * ((p * WORDS + c) % 4))) & 255u);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < NC; ++c) px[p][c] = p < n_valid ? (int)row[p * step + c] : 0;
            }
        }
        for (int e = 0; e < total; ++e) {
            const int4 a = sh.list[e * 4];
            if (n_valid == 0 || y < a.y || y > a.w || xl < a.x || xf > a.z) continue;
            const int4 b = sh.list[e * 4 + 1], tg = sh.list[e * 4 + 2], cd = sh.list[e * 4 + 3];
            int col[NC], txt[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                col[c] = (int)(((unsigned)cd.x >> (8 * (pl.coff + c))) & 255u);
                txt[c] = (int)((text_colour >> (8 * (pl.coff + c))) & 255u);
            }
            const bool y_box = y >= b.y && y <= b.w, y_outer = y >= b.y - q.o && y <= b.w + q.o, y_inner = y >= b.y + q.i && y <= b.w - q.i;
            const int ty = y - tg.y;
            const bool y_tag = tg.z > 0 && ty >= 0 && ty < 9 * q.scale;
            const int gy = y_tag ? ty / q.scale - 1 : -1;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int x = xf + (p << pl.sub);
                if (p >= n_valid || x < a.x || x > a.z) continue;
                if (q.alpha > 0 && y_box && x >= b.x && x <= b.z) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) px[p][c] = (px[p][c] * (256 - q.alpha) + col[c] * q.alpha + 128) >> 8;
                    dirty |= 1u << p;
                }
                if (y_outer && x >= b.x - q.o && x <= b.z + q.o && !(y_inner && x >= b.x + q.i && x <= b.z - q.i)) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) px[p][c] = col[c];
                    dirty |= 1u << p;
                }
                const int tx = x - tg.x;
                if (y_tag && tx >= 0 && tx < tg.z) {
                    const int gx = tx / q.scale - 1;
                    bool on = false;
                    if (gy >= 0 && gy < 7 && gx >= 0) {
                        const int dq = gx / 6, dc = gx - dq * 6;
                        if (dq < tg.w && dc < 5) {
                            const unsigned long long dg = (unsigned long long)(unsigned)cd.y | (unsigned long long)(unsigned)cd.z << 32;
                            const int digit = (int)((dg >> (4 * dq)) & 15ull);
                            on = (GLYPHS[min(digit, 9)] >> (5 * gy + 4 - dc)) & 1ull;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < NC; ++c) px[p][c] = on ? txt[c] : col[c];
                    dirty |= 1u << p;
                }
            }
        }
        __syncthreads();                         // the list is rewritten by the next step
    }
    if (!dirty) return;
    if (wide) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int at = p * WORDS + c;
                words[at / 4] = (words[at / 4] & ~(255u << (8 * (at % 4)))) | ((unsigned)px[p][c] << (8 * (at % 4)));
            }
#pragma unroll
        for (int e = 0; e < WORDS; ++e) ((gwords)row)[e] = words[e];
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (dirty >> p & 1u)
#pragma unroll
                for (int c = 0; c < NC; ++c) row[p * step + c] = (unsigned char)px[p][c];
    }
}

// packed C-channel frames (cnl_letterbox_frame): channels 0..2 are painted, a fourth is carried
template <int C>
struct PackedFormat {
    typedef cnl_letterbox_frame Frame;
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ void run(const Frame& f, const SlotRecord* recs, const Style& q, unsigned text, int tx, int ty, int,
                                               PaintShared& sh) {
        const Plane pl = {(unsigned char*)f.src, f.row_stride, C, f.w, f.h, 0, 0};
        paint<C, 3>(pl, recs, q, text, tx, ty, sh);
    }
};
// YUV 4:2:0 planes (cnl_yuv420_frame, the whole frame): plane 0 = Y; NV12: plane 1 = the interleaved UV samples; otherwise plane 1 = U
// and plane 2 = V, c_step bytes from one sample to the next
struct Yuv420Format {
    typedef cnl_yuv420_frame Frame;
    static constexpr int PLANES = 3;
    static __device__ __forceinline__ void run(const Frame& f, const SlotRecord* recs, const Style& q, unsigned text, int tx, int ty, int plane,
                                               PaintShared& sh) {
        if (plane == 0) {
            const Plane pl = {(unsigned char*)f.y, f.y_pitch, 1, f.w, f.h, 0, 0};
            paint<1, 1>(pl, recs, q, text, tx, ty, sh);
            return;
        }
        const bool interleaved = f.c_step == 2 && f.v == (const void*)((const unsigned char*)f.u + 1);
        if (interleaved) {
            if (plane == 1) {
                const Plane pl = {(unsigned char*)f.u, f.c_pitch, 2, f.w >> 1, f.h >> 1, 1, 1};
                paint<2, 2>(pl, recs, q, text, tx, ty, sh);
            }
            return;
        }
        const Plane pl = {(unsigned char*)(plane == 1 ? f.u : f.v), f.c_pitch, f.c_step, f.w >> 1, f.h >> 1, 1, plane};
        if (f.c_step == 1)
            paint<1, 1>(pl, recs, q, text, tx, ty, sh);
        else
            paint<0, 1>(pl, recs, q, text, tx, ty, sh);
    }
};

template <class Format>
__global__ __launch_bounds__(OV_THREADS) void overlay_paint_kernel(const typename Format::Frame* __restrict__ table,
                                                                   const SlotRecord* __restrict__ records,
                                                                   const unsigned* __restrict__ palette, Style q, int tiles_x) {
    __shared__ PaintShared sh;
    const typename Format::Frame f = table[blockIdx.y];          // uniform address: scalar loads
    const int tile_x = (int)(blockIdx.x % (unsigned)tiles_x), tile_y = (int)(blockIdx.x / (unsigned)tiles_x);
    const unsigned text_colour = palette[q.P];                   // the entry after the P slot colours
    Format::run(f, records + (size_t)blockIdx.y * q.k, q, text_colour, tile_x, tile_y, (int)blockIdx.z, sh);
}

template <class Format>
static int draw(const void* frames, const float* boxes, const int64_t* labels, const int32_t* numbers, const float* scores, const int32_t* count,
                const uint32_t* palette, void* records, int N, long total, const Style& q, int max_h, int max_w, void* stream) {
    typedef typename Format::Frame Frame;
    hipLaunchKernelGGL(overlay_records_kernel<Frame>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const Frame*>(frames), reinterpret_cast<const float4*>(boxes), reinterpret_cast<const long long*>(labels),
                       numbers, scores, count, palette, static_cast<SlotRecord*>(records), total, q);
    if (int e = cnl::check_launch("overlay_records_kernel")) return e;
    const int tiles_x = (max_w + OV_TILE_W - 1) / OV_TILE_W, tiles_y = (max_h + OV_TILE_H - 1) / OV_TILE_H;
    hipLaunchKernelGGL(overlay_paint_kernel<Format>, dim3((unsigned)(tiles_x * tiles_y), (unsigned)N, (unsigned)Format::PLANES), dim3(OV_THREADS), 0,
                       (hipStream_t)stream, static_cast<const Frame*>(frames), static_cast<const SlotRecord*>(records), palette, q, tiles_x);
    return cnl::check_launch("overlay_paint_kernel");
}

}  // namespace cnl_overlay

extern "C" int cnl_draw_boxes_u8(const void* frames, const float* boxes, const int64_t* labels, const int32_t* numbers, const float* scores,
                                 float score_threshold, const int32_t* count, int32_t N, int32_t k, int32_t C, int32_t yuv,
                                 const uint32_t* palette, int32_t P, int32_t thickness, int32_t fill_alpha, int32_t tag_scale,
                                 int32_t max_h, int32_t max_w, void* records, void* stream) {
    using namespace cnl_overlay;
    CNL_REQUIRE(N >= 0 && k >= 0, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: negative N or k");
    CNL_REQUIRE(N <= 65535, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: N = %d outside 0..65535", N);
    const long total = (long)N * k;
    CNL_REQUIRE(total <= 0x7fffffffL, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: N * k = %ld slots exceed 2^31 - 1", total);
    CNL_REQUIRE(yuv ? C == 3 : (C == 3 || C == 4), CNL_E_BAD_ARG, "cnl_draw_boxes_u8: C = %d (packed frames have 3 or 4 channels, YUV frames 3)", C);
    CNL_REQUIRE(P >= 1 && P <= 256, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: P = %d palette entries outside 1..256", P);
    CNL_REQUIRE(thickness >= 1 && thickness <= 32, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: thickness = %d outside 1..32", thickness);
    CNL_REQUIRE(fill_alpha >= 0 && fill_alpha <= 256, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: fill_alpha = %d outside 0..256", fill_alpha);
    CNL_REQUIRE(tag_scale >= 0 && tag_scale <= 8, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: tag_scale = %d outside 0..8", tag_scale);
    CNL_REQUIRE(!scores || score_threshold == score_threshold, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: score_threshold is NaN");
    if (total == 0) return CNL_OK;               // no slots: nothing is painted and the pointers are not looked at
    CNL_REQUIRE(max_h >= 1 && max_h <= 32768 && max_w >= 1 && max_w <= 32768, CNL_E_BAD_ARG,
                "cnl_draw_boxes_u8: largest frame %d x %d outside 1..32768", max_h, max_w);
    CNL_REQUIRE(frames && boxes && palette && records, CNL_E_BAD_ARG, "cnl_draw_boxes_u8: null pointer");
    CNL_REQUIRE(((uintptr_t)frames & 7) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)boxes & 15) == 0 && ((uintptr_t)records & 15) == 0 &&
                    ((uintptr_t)palette & 3) == 0 && ((uintptr_t)numbers & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)count & 3) == 0,
                CNL_E_BAD_ARG,
                "cnl_draw_boxes_u8: frames and labels must be 8-byte, boxes and records 16-byte, palette, numbers, scores and count 4-byte aligned");
    const int o = (thickness - 1) / 2;
    const Style q = {k, P, thickness, o, thickness - o, fill_alpha, tag_scale, score_threshold};
    if (yuv) return draw<Yuv420Format>(frames, boxes, labels, numbers, scores, count, palette, records, N, total, q, max_h, max_w, stream);
    if (C == 3) return draw<PackedFormat<3>>(frames, boxes, labels, numbers, scores, count, palette, records, N, total, q, max_h, max_w, stream);
    return draw<PackedFormat<4>>(frames, boxes, labels, numbers, scores, count, palette, records, N, total, q, max_h, max_w, stream);
}
