// loss_common.h — the ONE copy of what det_loss.hip and reid_loss.hip both do around their own arithmetic:
//   the tile constants   256 threads own an 8 x 32 pixel tile of one image; PASS_SLOTS target slots are staged per pass, MAX_G per image
//   Tile / element       blockIdx.x -> (image, pixel rectangle), and the element (x, y, channel) a thread handles in a step of a tile walk
//   stage_pass           ordered compaction: the slots of one pass that a predicate accepts, written to LDS in slot order
//   block_sum_fixed      a workgroup's float64 sum in a fixed tree
//   check_dims ...       the bounds every entry point and every *_workspace_bytes shares, and the checks of alignment, workspace and grid
// A kernel file says `using namespace cnl_loss;` inside its own namespace and keeps its kernels, records and arithmetic.
#pragma once
#include "cnl_common.h"

#pragma clang fp contract(off)   // one rounding per operation

namespace cnl_loss {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TILE_W = 32, TILE_H = 8;             // TILE_W * TILE_H == THREADS: every thread of a tile makes the same number of element steps
constexpr int PASS_SLOTS = 256;                    // target slots staged per pass (one per thread)
constexpr int MAX_G = 1024;                        // boxes per image
constexpr int MAX_N = 1 << 16, MAX_SIDE = 1 << 15; // images per call, map height and width
constexpr double MAX_STRIDE = 1e6;
static_assert(TILE_W * TILE_H == THREADS && PASS_SLOTS == THREADS, "one element / one slot per thread and step");

enum { LAYOUT_CMINOR = 0, LAYOUT_PLANE = 1, LAYOUT_GENERIC = 2 };

__host__ __device__ inline int tiles_x(int W) { return (W + TILE_W - 1) / TILE_W; }
__host__ __device__ inline int tiles_y(int H) { return (H + TILE_H - 1) / TILE_H; }

// the tile of workgroup `block` of a grid of N * tiles_x * tiles_y: image n, pixels [x0, x1) x [y0, y1)
struct Tile {
    int n, x0, y0, x1, y1;
    __device__ __forceinline__ Tile(unsigned block, int tx, int H, int W) {
        const int tiles = tx * tiles_y(H);
        n = block / tiles;
        const int tile = block - n * tiles, ty = tile / tx, txi = tile - ty * tx;
        x0 = txi * TILE_W; y0 = ty * TILE_H; x1 = min(x0 + TILE_W, W); y1 = min(y0 + TILE_H, H);
    }
    __device__ __forceinline__ bool holds(int x, int y) const { return x < x1 && y < y1; }      // (x >= x0 and y >= y0 by construction)
};

// The element of thread tid in step `step` of a walk over a tile's THREADS * C elements (C steps in every thread, so barriers inside a step are
// uniform).  Channel-minor: lanes along the channels of a pixel, then along x.  Plane: lanes along x, then y; one channel per step.
struct Elem { int x, y, c; };
__device__ __forceinline__ Elem element(bool cminor, const Tile& t, int step, int C) {
    const int tid = threadIdx.x;
    Elem e;
    if (cminor) {
        const unsigned row = (unsigned)TILE_W * (unsigned)C;
        const unsigned i = (unsigned)step * THREADS + (unsigned)tid;
        const unsigned yy = i / row, j = i - yy * row, xx = j / (unsigned)C;
        e.y = t.y0 + (int)yy; e.x = t.x0 + (int)xx; e.c = (int)(j - xx * (unsigned)C);
    } else {
        e.c = step; e.y = t.y0 + tid / TILE_W; e.x = t.x0 + tid % TILE_W;
    }
    return e;
}

__device__ __forceinline__ double wave_sum_fixed(double v) {      // the same tree in every lane, every run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// sum over the workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_fixed(double v, double* s_part) {
    v = wave_sum_fixed(v);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = s_part[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += s_part[w];
    __syncthreads();
    return s;
}

// The place of this thread's hit among the workgroup's hits in thread order, and how many there are: ballot, a popcount per wave into s_cnt, a
// barrier, the prefix over the waves.  (A plain function: the amdgcn builtins stay out of templates, see cnl_device.h.)
__device__ __forceinline__ int ordered_slot(bool hit, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(votes);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int c = s_cnt[w];
        if (w < wave) base += c;
        total += c;
    }
    return base + __popcll(votes & ((1ull << lane) - 1ull));
}

// One staging pass, called by every thread: thread tid asks pick(s, v) whether slot s = s0 + tid (of n slots) is wanted (pick fills v); the wanted
// values land in s_out[0 .. count) in slot order -> count.  Three barriers: the readers of the previous pass are done, the counts are written,
// the values are written.  s_cnt: WAVES ints of LDS.  (The bound is tested here, not in pick: every load of pick is then waited for on one path,
// and no vmcnt(0) is left for the caller's next loop, where it would also wait for loads the caller issued early.)
template <class V, class F>
__device__ __forceinline__ int stage_pass(int s0, int n, V* s_out, int* s_cnt, F pick) {
    __syncthreads();
    const int s = s0 + (int)threadIdx.x;
    bool hit = false;
    V v;
    if (s < n) hit = pick(s, v);
    int total;
    const int slot = ordered_slot(hit, s_cnt, total);
    if (hit) s_out[slot] = v;
    __syncthreads();
    return total;
}

// ---------------------------------------------------------------------------------------------------------------- host
inline bool slots_in_range(int N, int Gmax) { return N >= 0 && N <= MAX_N && Gmax >= 1 && Gmax <= MAX_G; }
inline bool dims_in_range(int N, int Gmax, int H, int W) { return slots_in_range(N, Gmax) && H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE; }
inline int check_dims(const char* who, int N, int H, int W, int Gmax) {
    CNL_REQUIRE(N >= 0 && N <= MAX_N, CNL_E_BAD_ARG, "%s: N = %d outside 0..2^16", who, N);
    CNL_REQUIRE(H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE, CNL_E_BAD_ARG, "%s: H x W = %d x %d outside 1..2^15", who, H, W);
    CNL_REQUIRE(Gmax >= 1 && Gmax <= MAX_G, CNL_E_BAD_ARG, "%s: Gmax = %d outside 1..%d", who, Gmax, MAX_G);
    return CNL_OK;
}
inline int check_stride(const char* who, double stride) {
    CNL_REQUIRE(stride > 0.0 && stride < MAX_STRIDE, CNL_E_BAD_ARG, "%s: stride = %g must be positive", who, stride);
    return CNL_OK;
}
// alignment of a call's pointers (NULL passes): the float64 / int64 arrays, the workspace, the fp32 / int32 arrays
inline int check_aligned(const char* who, std::initializer_list<const void*> by8, const void* workspace, std::initializer_list<const void*> by4) {
    uintptr_t a8 = 0, a4 = 0;
    for (const void* p : by8) a8 |= (uintptr_t)p;
    for (const void* p : by4) a4 |= (uintptr_t)p;
    CNL_REQUIRE((a8 & 7) == 0 && ((uintptr_t)workspace & 15) == 0 && (a4 & 3) == 0, CNL_E_BAD_ARG,
                "%s: a misaligned pointer (float64 / int64 arrays: 8-byte aligned, a workspace: 16-byte aligned, the rest: 4-byte aligned)", who);
    return CNL_OK;
}
inline int check_workspace(const char* who, size_t have, size_t need) {
    CNL_REQUIRE(have >= need, CNL_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, have, need);
    return CNL_OK;
}
// -> tiles per image in `tiles`; N * tiles workgroups must fit a grid
inline int check_tile_grid(const char* who, int N, int H, int W, int& tiles) {
    tiles = tiles_x(W) * tiles_y(H);
    CNL_REQUIRE((long long)N * tiles < (1ll << 31), CNL_E_UNSUPPORTED, "%s: %d images x %d tiles exceed the grid", who, N, tiles);
    return CNL_OK;
}

}  // namespace cnl_loss
