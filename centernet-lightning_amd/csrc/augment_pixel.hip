// augment_pixel.hip — the pixel-level training augmentation of a batch of FINISHED canvases on the device: the transforms of the
// reference's training lists that need a neighbourhood or a histogram — MotionBlur and Sharpen (one FILTER of up to 32 integer taps), Posterize,
// Solarize and Equalize (one 256-entry table per channel) — ONE operation per canvas, then that canvas's holes.  Integers only: the rule is the
// header's (cnl_augment_pixel_u8) and tests/pixel_ref.py restates it.
//
//   hist_kernel    only when the plan holds an EQUALIZE: a workgroup owns blocks of LB_ROWS whole canvas rows, counts their bytes into an LDS
//                  histogram of 3 x 256 (eight counters per bin) with integer LDS atomics and writes it to its own slot of the workspace (no
//                  global atomics, no memset; the sum of integers does not depend on the order of the adds)
//   lut_kernel     one workgroup per canvas: sums the slots in slot order and builds the three 256-byte tables of EQUALIZE by the header's
//                  64-bit rule, or writes POSTERIZE's / SOLARIZE's
//   apply_kernel   the canvas tiling of the other pixel kernels (CanvasGrid: blocks of LB_ROWS rows x column tiles of <= 1024 columns), one
//                  uniform branch per canvas: a table canvas maps its 4-pixel groups through the 768 bytes in LDS; a FILTER canvas stages
//                  chunks of FILTER_CHUNK columns plus the canvas's OWN halo (rx, ry <= 15, the largest |dx|, |dy| of its taps) into LDS as one
//                  word per pixel with the reflection applied at staging, then walks the taps (uniform: broadcast LDS reads); NONE copies.
//                  Then find_holes / punch (augment_common.h) and the 4-pixel group stores: every output byte is written exactly once.
//
// LDS of apply_kernel: (LB_ROWS + 30) x (FILTER_CHUNK + 30) words = 43,472 bytes for the stage, 768 for the tables, 512 for the taps, 260 for the
// holes: 45,012 bytes, three workgroups (12 waves) per CU of 160 KiB.  A horizontal blur (ry = 0) re-reads nothing vertically; a filter of full
// radius reads (8 + 30) / 8 = 4.75 times its rows, from L2.
#include "augment_common.h"

namespace cnl_augment {

static_assert(sizeof(cnl_pixel_op) == 400 && offsetof(cnl_pixel_op, taps) == 16, "cnl_pixel_op's layout");

constexpr int PIXEL_MAX_TAPS = CNL_PIXEL_MAX_TAPS, PIXEL_RADIUS = CNL_PIXEL_MAX_RADIUS;
constexpr int HIST_PARTS = 32;                   // histogram slots per canvas at most
constexpr int HIST_COPIES = 8;                   // counters per bin in a workgroup's LDS histogram (a power of two): 24 KB
constexpr int HIST_LOADS = 8;                    // histogram words a thread has in flight before it counts them
constexpr int FILTER_CHUNK = 256;               // canvas columns staged at once
constexpr int STAGE_PITCH = FILTER_CHUNK + 2 * PIXEL_RADIUS, STAGE_ROWS = LB_ROWS + 2 * PIXEL_RADIUS;
constexpr long long FILTER_ABS_MAX = 1ll << 23;  // sum |w|: 255 * 2^23 + 2^15 < 2^31
static_assert(FILTER_CHUNK % 4 == 0 && LB_THREADS == 256, "a chunk is whole groups; one thread per table entry");

static inline int hist_parts(int height) { return min((height + LB_ROWS - 1) / LB_ROWS, HIST_PARTS); }

// the table operation of a record, or CNL_PIXEL_NONE when it has none or its parameter is out of range
__device__ __forceinline__ int table_op(int op, int param) {
    if (op == CNL_PIXEL_POSTERIZE) return param >= 0 && param <= 8 ? op : CNL_PIXEL_NONE;
    if (op == CNL_PIXEL_SOLARIZE) return param >= 0 && param <= 255 ? op : CNL_PIXEL_NONE;
    return op == CNL_PIXEL_EQUALIZE ? op : CNL_PIXEL_NONE;
}

// cv2's BORDER_REFLECT_101 made total: any i, n >= 1
__device__ __forceinline__ int reflect101(int i, int n) {
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}

// the 12 bytes of a group as three words <-> pixel p's three channel bytes, channel c at bits 8c (store_group's inverse)
__device__ __forceinline__ void load_group3(const unsigned* src, unsigned (&px)[4]) {
    const unsigned w0 = src[0], w1 = src[1], w2 = src[2];
    px[0] = w0 & 0xffffffu;
    px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
    px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
    px[3] = w2 >> 8;
}

__global__ __launch_bounds__(LB_THREADS) void hist_kernel(const unsigned* __restrict__ canvas, const cnl_pixel_op* __restrict__ ops, int height, int width,
                                                          int parts, unsigned* __restrict__ partial) {
    // HIST_COPIES counters per bin, one per lane of a group of neighbours: neighbouring pixels hold similar values, and lanes of one wave that
    // add to the same address take turns
    __shared__ unsigned hist[768 * HIST_COPIES];
    const int n = (int)blockIdx.y, part = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (table_op(ops[n].op, ops[n].param) != CNL_PIXEL_EQUALIZE) return;       // uniform: this canvas's slots are never read
    for (int k = tid; k < 768 * HIST_COPIES; k += LB_THREADS) hist[k] = 0;
    __syncthreads();
    unsigned* const mine = hist + (tid & (HIST_COPIES - 1));
    const int row_words = width / 4 * 3;                                        // a row is whole words: width % 4 == 0
    const unsigned* const base = canvas + (size_t)n * height * row_words;
    const int row_blocks = (height + LB_ROWS - 1) / LB_ROWS;
    for (int rb = part; rb < row_blocks; rb += parts) {
        const int row_begin = rb * LB_ROWS, n_rows = min(LB_ROWS, height - row_begin);
        const int first = row_begin * row_words, words = n_rows * row_words;   // height * width * 3 <= 2^31 - 1: fits
        for (int i0 = tid; i0 < words; i0 += HIST_LOADS * LB_THREADS) {         // HIST_LOADS loads in flight per thread, then their adds
            unsigned w[HIST_LOADS];
#pragma unroll
            for (int u = 0; u < HIST_LOADS; ++u) {
                const int i = i0 + u * LB_THREADS;
                w[u] = i < words ? base[first + i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < HIST_LOADS; ++u) {
                const int i = i0 + u * LB_THREADS;
                if (i >= words) break;
                const int c0 = i % 3;                                           // byte 4 i of the block is channel (4 i) % 3 = i % 3
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int c = (c0 + b) % 3;
                    atomicAdd(&mine[(c * 256 + (int)((w[u] >> (8 * b)) & 255u)) * HIST_COPIES], 1u);
                }
            }
        }
    }
    __syncthreads();
    unsigned* const slot = partial + ((size_t)n * parts + part) * 768;
    for (int k = tid; k < 768; k += LB_THREADS) {
        unsigned s = 0;
#pragma unroll
        for (int r = 0; r < HIST_COPIES; ++r) s += hist[k * HIST_COPIES + r];
        slot[k] = s;
    }
}

__global__ __launch_bounds__(LB_THREADS) void lut_kernel(const cnl_pixel_op* __restrict__ ops, int height, int width, int parts, int with_hist,
                                                         const unsigned* __restrict__ partial, unsigned char* __restrict__ lut) {
    __shared__ unsigned hist[768];               // the histogram, then cum(v) of the populated part above the first bin
    __shared__ int first_bin[3];
    __shared__ unsigned first_count[3];
    const int n = (int)blockIdx.x, v = (int)threadIdx.x;
    const int param = ops[n].param;
    int op = table_op(ops[n].op, param);
    if (op == CNL_PIXEL_EQUALIZE && !with_hist) op = CNL_PIXEL_NONE;             // no histogram was launched: the identity table
    unsigned char* const dst = lut + (size_t)n * 768;
    if (op != CNL_PIXEL_EQUALIZE) {
        int t = v;
        if (op == CNL_PIXEL_POSTERIZE) t = v & (0xff << (8 - param)) & 0xff;
        if (op == CNL_PIXEL_SOLARIZE) t = v >= param ? 255 - v : v;
        dst[v] = dst[256 + v] = dst[512 + v] = (unsigned char)t;
        return;
    }
    const unsigned* const slots = partial + (size_t)n * parts * 768;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned s = 0;
        for (int p = 0; p < parts; ++p) s += slots[(size_t)p * 768 + c * 256 + v];
        hist[c * 256 + v] = s;
    }
    __syncthreads();
    if (v < 3) {                                 // 256 adds: not worth a scan
        unsigned* const h = hist + v * 256;
        int i0 = 0;
        while (i0 < 255 && h[i0] == 0) ++i0;
        first_bin[v] = i0;
        first_count[v] = h[i0];
        unsigned cum = 0;
        for (int i = 0; i < 256; ++i) {
            cum = i <= i0 ? 0u : cum + h[i];
            h[i] = cum;
        }
    }
    __syncthreads();
    const long long total = (long long)height * width;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long d = total - (long long)first_count[c];
        int t = v;
        if (d > 0) t = v <= first_bin[c] ? 0 : (int)((510ll * (long long)hist[c * 256 + v] + d) / (2 * d));
        dst[c * 256 + v] = (unsigned char)t;     // cum <= d: at most 255
    }
}

__global__ __launch_bounds__(LB_THREADS) void apply_kernel(const unsigned char* __restrict__ canvas, const cnl_pixel_op* __restrict__ ops,
                                                           const int4* __restrict__ holes, const unsigned char* __restrict__ lut,
                                                           unsigned char* __restrict__ out, int height, int width, int with_lut, unsigned hole_fill,
                                                           int tiles_x, int groups_per_tile) {
    __shared__ unsigned stage[STAGE_ROWS * STAGE_PITCH];
    __shared__ unsigned table[192];              // 3 x 256 bytes
    __shared__ int4 tap[PIXEL_MAX_TAPS];         // (dx, dy, w, 0)
    __shared__ int4 hole[MAX_HOLES];
    __shared__ unsigned hole_mask;

    const int n = (int)blockIdx.y;
    const int tile = (int)(blockIdx.x % (unsigned)tiles_x), rblk = (int)(blockIdx.x / (unsigned)tiles_x);
    const int groups = width >> 2;
    const int g_begin = tile * groups_per_tile, g_end = min(groups, g_begin + groups_per_tile);
    const int n_groups = g_end - g_begin;
    const int x_begin = g_begin * 4, x_end = g_end * 4;
    const int row_begin = rblk * LB_ROWS, n_rows = min(LB_ROWS, height - row_begin), row_end = row_begin + n_rows;
    const int tid = (int)threadIdx.x;

    const cnl_pixel_op* const q = ops + n;       // uniform address: scalar loads
    int op = q->op;
    const int n_taps = q->n_taps;
    if (op == CNL_PIXEL_FILTER) {
        if (n_taps < 1 || n_taps > PIXEL_MAX_TAPS) op = CNL_PIXEL_NONE;
    } else {
        op = with_lut ? table_op(op, q->param) : CNL_PIXEL_NONE;
    }
    if (op == CNL_PIXEL_FILTER && tid < n_taps) tap[tid] = make_int4(q->taps[tid][0], q->taps[tid][1], q->taps[tid][2], 0);
    if (op >= CNL_PIXEL_POSTERIZE && tid >= 64 && tid < 64 + 192) table[tid - 64] = reinterpret_cast<const unsigned*>(lut + (size_t)n * 768)[tid - 64];
    if (tid < 64) find_holes(holes, n, tid, width, height, x_begin, x_end, row_begin, row_end, hole, hole_mask);      // the first wave
    __syncthreads();

    // a FILTER record with an offset beyond +-15 or sum |w| > 2^23 runs as NONE: judged by every thread alike, so nothing can index out of the stage
    int rx = 0, ry = 0;
    if (op == CNL_PIXEL_FILTER) {
        long long abs_sum = 0;
        bool bad = false;
        for (int t = 0; t < n_taps; ++t) {
            const int4 e = tap[t];
            bad = bad || e.x < -PIXEL_RADIUS || e.x > PIXEL_RADIUS || e.y < -PIXEL_RADIUS || e.y > PIXEL_RADIUS;
            rx = max(rx, abs(min(max(e.x, -PIXEL_RADIUS), PIXEL_RADIUS)));
            ry = max(ry, abs(min(max(e.y, -PIXEL_RADIUS), PIXEL_RADIUS)));
            abs_sum += e.z < 0 ? -(long long)e.z : (long long)e.z;
        }
        if (bad || abs_sum > FILTER_ABS_MAX) op = CNL_PIXEL_NONE;
    }

    const unsigned touching = (unsigned)__builtin_amdgcn_readfirstlane((int)hole_mask);
    const size_t plane = (size_t)n * height * width * 3;
    const unsigned char* const src = canvas + plane;
    unsigned char* const dst = out + plane;

    if (op != CNL_PIXEL_FILTER) {
        const unsigned char* const tb = reinterpret_cast<const unsigned char*>(table);
        const int items = n_rows * n_groups;
        for (int i = tid; i < items; i += LB_THREADS) {
            const int r = i / n_groups, g = i - r * n_groups;
            const int y = row_begin + r, x = x_begin + g * 4;
            const size_t at = ((size_t)y * width + (size_t)x) * 3;
            unsigned px[4];
            load_group3(reinterpret_cast<const unsigned*>(src + at), px);
            if (op != CNL_PIXEL_NONE) {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    px[p] = (unsigned)tb[px[p] & 255u] | ((unsigned)tb[256 + ((px[p] >> 8) & 255u)] << 8) | ((unsigned)tb[512 + (px[p] >> 16)] << 16);
            }
            punch(touching, hole, y, x, hole_fill, px);
            store_group<3>(reinterpret_cast<unsigned*>(dst + at), px);
        }
        return;
    }

    for (int cx0 = x_begin; cx0 < x_end; cx0 += FILTER_CHUNK) {                  // uniform: every thread meets every barrier
        const int cw = min(x_end, cx0 + FILTER_CHUNK) - cx0;
        const int sw = cw + 2 * rx, sh = n_rows + 2 * ry;                        // <= STAGE_PITCH, <= STAGE_ROWS
        if (cx0 != x_begin) __syncthreads();                                     // the last chunk's taps have been read
        for (int i = tid; i < sw * sh; i += LB_THREADS) {
            const int j = i / sw, k = i - j * sw;                               // j < sh <= STAGE_ROWS, k < sw <= STAGE_PITCH
            const int sy = reflect101(row_begin - ry + j, height), sx = reflect101(cx0 - rx + k, width);
            const unsigned char* const p = src + ((size_t)sy * width + (size_t)sx) * 3;
            stage[j * STAGE_PITCH + k] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
        }
        __syncthreads();
        const int cg = cw >> 2, items = n_rows * cg;
        for (int i = tid; i < items; i += LB_THREADS) {
            const int r = i / cg, g = i - r * cg;
            const int y = row_begin + r, x = cx0 + g * 4;
            int acc[4][3];
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 32768;
            const int base = (r + ry) * STAGE_PITCH + g * 4 + rx;
            for (int t = 0; t < n_taps; ++t) {
                const int4 e = tap[t];                                           // |e.x| <= rx, |e.y| <= ry
                const unsigned* const s = stage + base + e.y * STAGE_PITCH + e.x;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const unsigned v = s[p];
                    acc[p][0] += e.z * (int)(v & 255u);
                    acc[p][1] += e.z * (int)((v >> 8) & 255u);
                    acc[p][2] += e.z * (int)(v >> 16);
                }
            }
            unsigned px[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                unsigned v = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int t = acc[p][c] >> 16;
                    asm volatile("" : "+v"(t));                                  // opaque before the clamp: colour_step's lesson (augment_common.h)
                    v |= (unsigned)min(max(t, 0), 255) << (8 * c);
                }
                px[p] = v;
            }
            punch(touching, hole, y, x, hole_fill, px);
            store_group<3>(reinterpret_cast<unsigned*>(dst + ((size_t)y * width + (size_t)x) * 3), px);
        }
    }
}

}  // namespace cnl_augment

extern "C" size_t cnl_augment_pixel_workspace_bytes(int32_t N, int32_t height, int32_t width) {
    using namespace cnl_augment;
    if (N < 1 || N > 65535 || height < 1 || height > 32768 || width < 4 || width > 32768) return 0;
    return (size_t)N * 768 + (size_t)N * hist_parts(height) * 768 * sizeof(unsigned);
}

extern "C" int cnl_augment_pixel_u8(const uint8_t* canvas, int32_t N, int32_t height, int32_t width, const void* ops, int32_t launches, const int32_t* holes,
                                    uint32_t hole_fill_rgba, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace cnl_augment;
    const char* entry = "cnl_augment_pixel_u8";
    CNL_REQUIRE(N >= 0 && N <= 65535, CNL_E_BAD_ARG, "%s: N = %d outside 0..65535", entry, N);
    CNL_REQUIRE((launches & ~(CNL_PIXEL_HAS_TABLE | CNL_PIXEL_HAS_EQUALIZE)) == 0 && (!(launches & CNL_PIXEL_HAS_EQUALIZE) || (launches & CNL_PIXEL_HAS_TABLE)),
                CNL_E_BAD_ARG, "%s: launches = %d must be 0, CNL_PIXEL_HAS_TABLE or CNL_PIXEL_HAS_TABLE | CNL_PIXEL_HAS_EQUALIZE", entry, launches);
    CNL_REQUIRE(height >= 1 && height <= 32768 && width >= 4 && width <= 32768 && width % 4 == 0, CNL_E_BAD_ARG,
                "%s: canvas %d x %d needs a height in 1..32768 and a width in 4..32768 that is a multiple of 4", entry, height, width);
    CNL_REQUIRE((long)height * width * 3 <= 0x7fffffffL, CNL_E_BAD_ARG, "%s: one canvas exceeds 2 GiB", entry);
    if (N == 0) return CNL_OK;                   // an empty batch is a no-op: its pointers are not looked at
    CNL_REQUIRE(canvas && ops && out, CNL_E_BAD_ARG, "%s: null pointer", entry);
    CNL_REQUIRE(((uintptr_t)canvas & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)ops & 3) == 0 && ((uintptr_t)holes & 15) == 0, CNL_E_BAD_ARG,
                "%s: canvas, out and ops must be 4-byte and holes 16-byte aligned", entry);
    const size_t bytes = (size_t)N * height * width * 3, need = cnl_augment_pixel_workspace_bytes(N, height, width);
    CNL_REQUIRE((uintptr_t)out >= (uintptr_t)canvas + bytes || (uintptr_t)canvas >= (uintptr_t)out + bytes, CNL_E_BAD_ARG,
                "%s: out must not alias canvas (a FILTER reads its neighbours)", entry);
    CNL_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, CNL_E_BAD_ARG, "%s: workspace must be given and 16-byte aligned", entry);
    CNL_REQUIRE(workspace_bytes == need, CNL_E_WORKSPACE, "%s: workspace_bytes = %zu, cnl_augment_pixel_workspace_bytes(%d, %d, %d) = %zu", entry,
                workspace_bytes, N, height, width, need);
    const cnl_pixel_op* const op = static_cast<const cnl_pixel_op*>(ops);
    unsigned char* const lut = static_cast<unsigned char*>(workspace);
    unsigned* const partial = reinterpret_cast<unsigned*>(lut + (size_t)N * 768);
    const int parts = hist_parts(height);
    if (launches & CNL_PIXEL_HAS_EQUALIZE) {
        hipLaunchKernelGGL(hist_kernel, dim3((unsigned)parts, (unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream,
                           reinterpret_cast<const unsigned*>(canvas), op, height, width, parts, partial);
        if (int e = cnl::check_launch("pixel hist_kernel")) return e;
    }
    if (launches & CNL_PIXEL_HAS_TABLE) {
        hipLaunchKernelGGL(lut_kernel, dim3((unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream, op, height, width, parts,
                           (launches & CNL_PIXEL_HAS_EQUALIZE) ? 1 : 0, partial, lut);
        if (int e = cnl::check_launch("pixel lut_kernel")) return e;
    }
    const CanvasGrid grid(height, width);
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)(grid.tiles_x * grid.row_blocks), (unsigned)N), dim3(LB_THREADS), 0, (hipStream_t)stream, canvas, op,
                       reinterpret_cast<const int4*>(holes), lut, out, height, width, (launches & CNL_PIXEL_HAS_TABLE) ? 1 : 0, hole_fill_rgba & 0xffffffu,
                       grid.tiles_x, grid.groups_per_tile);
    return cnl::check_launch("pixel apply_kernel");
}
