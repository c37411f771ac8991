// camera_motion.hip — the global image translation between a stream's previous and current frame (include/centernet_gfx950.h:
// cnl_camera_motion_u8), the estimate behind TrackerBank's camera_motion= option.  Integer arithmetic throughout; the rule is the header's and
// tests/camera_motion_ref.py restates it in numpy.
//
//   coarse_kernel<STEP, D>  the read-once stream: every frame's luma, box-averaged d x d into the stream's dense coarse plane.  grid.y = frame
//                           record, grid.x = strips of coarse rows (the record is read through a uniform pointer; a frame of any size costs
//                           its own rows and nothing else).  A thread owns 16 neighbouring source pixels of d rows: STEP unaligned 16-byte loads
//                           per row, 16 / d coarse bytes out.  The row's ragged end takes byte loads.
//   search_kernel<B>        one workgroup per (stream, block): the (B + 2R)^2 window of the previous plane and the B^2 block of the current one
//                           in LDS, one candidate shift per lane ((2R + 1)^2 <= 289 lanes of 320), SADs on packed bytes (v_sad_u8 on dwords,
//                           v_alignbyte_b32 for the unaligned window rows), the key (SAD, |sy| + |sx|, sy, sx) packed into 64 bits and
//                           minimised over the wave by shuffles, across the five waves through LDS.
//   aggregate_kernel        one workgroup per stream: the lower median of the votes per axis, by counting ranks over at most 256 votes.
// No atomics, no floats before the final conversion; every global write is a plain store with one writer.
#include <algorithm>
#include "cnl_common.h"

namespace cnl_motion {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));
typedef const __attribute__((address_space(1))) unsigned char* gbytes;
typedef const __attribute__((address_space(1))) u32x4_unaligned* gquads;

static_assert(sizeof(cnl_motion_frame) == 40 && sizeof(cnl_camera_motion) == 112, "record sizes of the header");

constexpr int COARSE_THREADS = 256, SEARCH_THREADS = 320, MAX_BLOCKS = 256;
constexpr int MAX_R = 8, MAX_B = 16, MAX_W = MAX_B + 2 * MAX_R;       // window side
constexpr int MAX_WP = MAX_W + 4;                                     // window row pitch: one dword of slack for the unaligned reads

constexpr int log2_of(int d) { return d == 1 ? 0 : 1 + log2_of(d >> 1); }

// luma of pixel p of a 16-pixel chunk held as STEP * 4 dwords (p is a compile-time constant after unrolling)
template <int STEP>
__device__ __forceinline__ int chunk_luma(const unsigned (&w)[STEP * 4], int p) {
    auto byte = [&](int b) { return (int)((w[b >> 2] >> (8 * (b & 3))) & 255u); };
    if (STEP == 1) return byte(p);
    return (77 * byte(p * STEP) + 150 * byte(p * STEP + 1) + 29 * byte(p * STEP + 2) + 128) >> 8;
}
template <int STEP>
__device__ __forceinline__ int pixel_luma(gbytes px) {
    if (STEP == 1) return px[0];
    return (77 * (int)px[0] + 150 * (int)px[1] + 29 * (int)px[2] + 128) >> 8;
}

template <int STEP, int D>
__global__ __launch_bounds__(COARSE_THREADS) void coarse_kernel(const cnl_motion_frame* __restrict__ frames) {
    constexpr int OUT = 16 / D;                                       // coarse pixels of a chunk
    const cnl_motion_frame f = frames[blockIdx.y];                    // uniform address: scalar loads
    const int Hc = f.h / D, Wc = f.w / D;
    if (Hc <= 0 || Wc <= 0) return;
    const int rows_per = (Hc + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = (int)blockIdx.x * rows_per, r1 = min(Hc, r0 + rows_per);
    if (r0 >= r1) return;
    const int used = Wc * D;                                          // source pixels of a row that count
    const int chunks = (used + 15) >> 4;
    const gbytes src = (gbytes)f.src;
    unsigned char* const cur = (unsigned char*)f.cur;
    const int items = (r1 - r0) * chunks;
    for (int i = threadIdx.x; i < items; i += COARSE_THREADS) {
        const int r = r0 + i / chunks, c = i % chunks;
        const int px0 = c * 16;
        const int n = min(16, used - px0);                            // pixels of this chunk that count: a multiple of D
        int acc[OUT];
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = 0;
        if (n == 16) {                                                // the 16 * STEP bytes lie inside the row
#pragma unroll
            for (int dy = 0; dy < D; ++dy) {
                const gbytes row = src + (size_t)(r * D + dy) * f.row_stride + (size_t)px0 * STEP;
                unsigned w[STEP * 4];
#pragma unroll
                for (int q = 0; q < STEP; ++q) {
                    const u32x4 v = ((gquads)row)[q];
                    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int p = 0; p < 16; ++p) acc[p / D] += chunk_luma<STEP>(w, p);
            }
        } else {
            for (int dy = 0; dy < D; ++dy) {
                const gbytes row = src + (size_t)(r * D + dy) * f.row_stride + (size_t)px0 * STEP;
#pragma unroll
                for (int p = 0; p < 16; ++p)
                    if (p < n) acc[p / D] += pixel_luma<STEP>(row + p * STEP);
            }
        }
        unsigned char* const out = cur + (size_t)r * Wc + (size_t)c * OUT;
        const int n_out = n / D;
#pragma unroll
        for (int o = 0; o < OUT; ++o)
            if (o < n_out) out[o] = (unsigned char)((acc[o] + (D * D) / 2) >> (2 * log2_of(D)));
    }
}

__host__ __device__ inline int block_start(int i, int m, int n, int R, int B) {
    const int span = n - 2 * R - B;
    return R + (m == 1 ? span / 2 : (int)(((long)i * span) / (m - 1)));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int B>
__global__ __launch_bounds__(SEARCH_THREADS) void search_kernel(const cnl_camera_motion a) {
    __shared__ __attribute__((aligned(16))) unsigned char win[MAX_W * MAX_WP + 16];
    __shared__ __attribute__((aligned(16))) unsigned char blk[B * B];
    __shared__ unsigned long long wave_key[SEARCH_THREADS / 64];
    const int tid = threadIdx.x, slot = blockIdx.y, b = blockIdx.x, nb = a.gy * a.gx;
    const cnl_motion_frame f = a.frames[slot];
    const int d = a.downscale, R = a.radius;
    const int Hc = f.h / d, Wc = f.w / d;
    short* const vec = a.vectors + ((size_t)slot * nb + b) * 2;
    int* const sad_out = a.sad + (size_t)slot * nb + b;
    if (f.prev == nullptr || Hc < 2 * R + B || Wc < 2 * R + B) {      // uniform: no previous plane, or a frame too small for the grid
        if (tid == 0) { vec[0] = 0; vec[1] = 0; *sad_out = -1; }
        return;
    }
    const int y0 = block_start(b / a.gx, a.gy, Hc, R, B), x0 = block_start(b % a.gx, a.gx, Wc, R, B);

    int masked = 0;                                                   // the block's centre pixel inside a live box
    if (a.boxes) {
        const float cx = (float)((x0 + B / 2) * d), cy = (float)((y0 + B / 2) * d);
        int live = a.k;
        if (a.count) live = min(max(a.count[slot], 0), a.k);
        const float* boxes = a.boxes + (size_t)slot * a.k * 4;
        for (int j = tid; j < live; j += SEARCH_THREADS) {
            const float x1 = boxes[4 * j], y1 = boxes[4 * j + 1], x2 = boxes[4 * j + 2], y2 = boxes[4 * j + 3];
            const bool finite = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
            if (finite && x1 <= cx && cx < x2 && y1 <= cy && cy < y2) masked = 1;
        }
    }

    const int W = B + 2 * R, WP = ((W + 3) & ~3) + 4;                 // rows start on dwords; the last dword of a row is slack
    const gbytes prev = (gbytes)f.prev, cur = (gbytes)f.cur;
    for (int i = tid; i < W * W; i += SEARCH_THREADS) {
        const int y = i / W, x = i - y * W;
        win[y * WP + x] = prev[(size_t)(y0 - R + y) * Wc + (x0 - R + x)];
    }
    for (int i = tid; i < B * B; i += SEARCH_THREADS) {
        const int y = i / B, x = i - y * B;
        blk[i] = cur[(size_t)(y0 + y) * Wc + (x0 + x)];
    }
    masked = __syncthreads_or(masked);

    int texture = 0;                                                  // wave 0: sum |cur - m|
    if (tid < 64) {
        const unsigned v = tid < B * B / 4 ? reinterpret_cast<const unsigned*>(blk)[tid] : 0u;
        const int total = wave_sum((int)__builtin_amdgcn_sad_u8(v, 0u, 0u));
        const unsigned m = (unsigned)((total + B * B / 2) / (B * B));
        texture = wave_sum(tid < B * B / 4 ? (int)__builtin_amdgcn_sad_u8(v, m * 0x01010101u, 0u) : 0);
    }

    const int side = 2 * R + 1;
    unsigned long long key = ~0ull;
    if (tid < side * side) {
        const int sy = tid / side - R, sx = tid % side - R;
        const int off = R - sx, sh = off & 3;                         // the block's row starts at byte `off` of a window row
        unsigned s = 0;
#pragma unroll
        for (int y = 0; y < B; ++y) {
            const unsigned* wr = reinterpret_cast<const unsigned*>(win + (y + R - sy) * WP) + (off >> 2);
            const unsigned* br = reinterpret_cast<const unsigned*>(blk + y * B);
            unsigned lo = wr[0];
#pragma unroll
            for (int j = 0; j < B / 4; ++j) {
                const unsigned hi = wr[j + 1];
                s = __builtin_amdgcn_sad_u8(br[j], __builtin_amdgcn_alignbyte(hi, lo, (unsigned)sh), s);
                lo = hi;
            }
        }
        key = ((unsigned long long)s << 32) | ((unsigned)(abs(sy) + abs(sx)) << 16) | ((unsigned)(sy + MAX_R) << 8) | (unsigned)(sx + MAX_R);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)key, o, 64), hi = __shfl_xor((unsigned)(key >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other < key ? other : key;
    }
    if ((tid & 63) == 0) wave_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < SEARCH_THREADS / 64; ++w) key = wave_key[w] < key ? wave_key[w] : key;
        const int best = (int)(key >> 32);
        const bool abstain = masked || texture < a.min_texture * B * B || best > a.max_sad * B * B;
        vec[0] = abstain ? (short)0 : (short)((int)(key & 255u) - MAX_R);
        vec[1] = abstain ? (short)0 : (short)((int)((key >> 8) & 255u) - MAX_R);
        *sad_out = abstain ? -1 : best;
    }
}

__global__ __launch_bounds__(MAX_BLOCKS) void aggregate_kernel(const cnl_camera_motion a) {
    __shared__ short vx[MAX_BLOCKS], vy[MAX_BLOCKS];
    __shared__ unsigned char voted[MAX_BLOCKS];
    __shared__ int median[2];
    const int tid = threadIdx.x, slot = blockIdx.x, nb = a.gy * a.gx;
    const cnl_motion_frame f = a.frames[slot];
    const int d = a.downscale, need = 2 * a.radius + a.block;
    const bool vote = tid < nb && a.sad[(size_t)slot * nb + tid] >= 0;
    const short sx = vote ? a.vectors[((size_t)slot * nb + tid) * 2] : (short)0, sy = vote ? a.vectors[((size_t)slot * nb + tid) * 2 + 1] : (short)0;
    vx[tid] = sx; vy[tid] = sy; voted[tid] = vote;
    if (tid < 2) median[tid] = 0;
    const int n = __syncthreads_count(vote);
    if (vote) {                                                      // the rank of this vote per axis: ties in block order
        int rx = 0, ry = 0;
        for (int j = 0; j < nb; ++j) {
            if (!voted[j]) continue;
            rx += vx[j] < sx || (vx[j] == sx && j < tid);
            ry += vy[j] < sy || (vy[j] == sy && j < tid);
        }
        if (rx == (n - 1) / 2) median[0] = sx;
        if (ry == (n - 1) / 2) median[1] = sy;
    }
    __syncthreads();
    if (tid == 0) {
        const bool few = n < a.min_blocks;
        a.shift[2 * slot] = few ? 0.f : (float)(median[0] * d);
        a.shift[2 * slot + 1] = few ? 0.f : (float)(median[1] * d);
        a.used[slot] = n;
        a.status[slot] = (f.prev == nullptr ? 1 : 0) | (few ? 2 : 0) | (f.h / d < need || f.w / d < need ? 4 : 0);
    }
}

typedef void (*coarse_fn)(const cnl_motion_frame*);
template <int STEP>
static coarse_fn coarse_for(int d) {
    return d == 1 ? coarse_kernel<STEP, 1> : d == 2 ? coarse_kernel<STEP, 2> : d == 4 ? coarse_kernel<STEP, 4> : coarse_kernel<STEP, 8>;
}

}  // namespace cnl_motion
using namespace cnl_motion;

extern "C" int cnl_camera_motion_u8(const cnl_camera_motion* p, int32_t stages, void* stream) {
    const char* name = "cnl_camera_motion_u8";
    CNL_REQUIRE(p, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(stages >= 1 && stages <= 7, CNL_E_BAD_ARG, "%s: stages = %d, expected 1 .. 7 (bit 0 coarse luma, bit 1 search, bit 2 aggregate)", name, stages);
    CNL_REQUIRE(p->frames && p->shift && p->used && p->vectors && p->sad && p->status, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(p->L >= 1 && p->k >= 0, CNL_E_BAD_ARG, "%s: L = %d, k = %d: expected L >= 1, k >= 0", name, p->L, p->k);
    CNL_REQUIRE(p->L <= 65535, CNL_E_UNSUPPORTED, "%s: L = %d > 65535 frames", name, p->L);
    CNL_REQUIRE(p->boxes ? p->k >= 1 : p->count == nullptr, CNL_E_BAD_ARG, "%s: boxes need k >= 1, and count needs boxes", name);
    CNL_REQUIRE(p->step == 1 || p->step == 3 || p->step == 4, CNL_E_BAD_ARG, "%s: step = %d, expected 1 (a luma plane), 3 or 4 bytes per pixel", name, p->step);
    const int d = p->downscale, B = p->block, R = p->radius;
    CNL_REQUIRE(d == 1 || d == 2 || d == 4 || d == 8, CNL_E_BAD_ARG, "%s: downscale = %d, expected 1, 2, 4 or 8", name, d);
    CNL_REQUIRE((B == 8 || B == 16) && R >= 1 && R <= MAX_R, CNL_E_BAD_ARG, "%s: block = %d, radius = %d: expected 8 or 16, and 1 .. 8", name, B, R);
    CNL_REQUIRE(p->gy >= 1 && p->gy <= 16 && p->gx >= 1 && p->gx <= 16, CNL_E_BAD_ARG, "%s: grid = %d x %d, expected 1 .. 16 each", name, p->gy, p->gx);
    CNL_REQUIRE(p->min_texture >= 0 && p->min_texture <= 255 && p->max_sad >= 0 && p->max_sad <= 255 && p->min_blocks >= 1, CNL_E_BAD_ARG,
                "%s: min_texture = %d, max_sad = %d, min_blocks = %d: expected 0 .. 255, 0 .. 255, >= 1", name, p->min_texture, p->max_sad, p->min_blocks);
    CNL_REQUIRE((((uintptr_t)p->shift | (uintptr_t)p->used | (uintptr_t)p->sad | (uintptr_t)p->status | (uintptr_t)p->boxes | (uintptr_t)p->count) & 3) == 0 &&
                ((uintptr_t)p->vectors & 1) == 0 && ((uintptr_t)p->frames & 7) == 0, CNL_E_BAD_ARG,
                "%s: shift, used, sad, status, boxes and count must be 4-byte aligned, vectors 2-byte aligned, frames 8-byte aligned", name);
    hipStream_t s = (hipStream_t)stream;
    if (stages & 1) {
        const coarse_fn fn = p->step == 1 ? coarse_for<1>(d) : p->step == 3 ? coarse_for<3>(d) : coarse_for<4>(d);
        const int strips = std::min(256, std::max(8, 2048 / p->L));
        hipLaunchKernelGGL(fn, dim3((unsigned)strips, (unsigned)p->L), dim3(COARSE_THREADS), 0, s, p->frames);
        if (int rc = cnl::check_launch("camera motion coarse_kernel")) return rc;
    }
    if (stages & 2) {
        const dim3 grid((unsigned)(p->gy * p->gx), (unsigned)p->L);
        if (B == 8) hipLaunchKernelGGL(search_kernel<8>, grid, dim3(SEARCH_THREADS), 0, s, *p);
        else hipLaunchKernelGGL(search_kernel<16>, grid, dim3(SEARCH_THREADS), 0, s, *p);
        if (int rc = cnl::check_launch("camera motion search_kernel")) return rc;
    }
    if (stages & 4) {
        hipLaunchKernelGGL(aggregate_kernel, dim3((unsigned)p->L), dim3(MAX_BLOCKS), 0, s, *p);
        if (int rc = cnl::check_launch("camera motion aggregate_kernel")) return rc;
    }
    return CNL_OK;
}
