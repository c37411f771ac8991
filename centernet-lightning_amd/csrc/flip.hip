// flip.hip — the flip test (test-time augmentation): the network also sees every image mirrored left-right, and the two sets of head
// outputs are averaged before the decode.  Two entry points, one launch each; the rule is stated in include/centernet_gfx950.h and
// restated in torch by tests/flip_ref.py.
//
//   cnl_mirror_append_u8   [N,H,W,C] uint8 -> [2N,H,W,C]: the images, then the images mirrored (the doubled network input).
//   cnl_flip_merge_f32     up to three head maps of the 2N forward -> merged[n,c,y,x] = 0.5f * (a[n,c,y,x] + b[n,p(c),y,W-1-x]).
//
// Both are pure memory traffic (the merge: two reads and one write per element, no reuse), so: no LDS, 16-byte accesses wherever the
// layout has 4 neighbouring elements, FLIP_UNROLL independent items per lane whose loads are all issued before the first store, and a
// grid sized to the chip (FLIP_WG_PER_CU workgroups per CU at most) that strides over the items.  A map's access form is chosen on the
// host from its strides and is the same for the whole map:
//   PIXEL4   every channel stride is 1 and C % 4 == 0 (what this package's forward produces): an item is 4 channels of one pixel, lanes
//            run along the pixel's channel vector; the mirrored operand is the same 4 channels of pixel W - 1 - x.  The box map's swap
//            of channels 0 and 2 is a component swap of its one vector.
//   ROW4     every column stride is 1 (contiguous NCHW): an item is 4 columns of one row; the mirrored operand's 4 columns are loaded
//            where they lie (W - 4 - x) and reversed in registers.  The W % 4 columns at the end of a row are single elements.
//   ELEMENT  anything else, one element per item, channels fastest when the destination's channel stride is its smallest.
// The 16-byte accesses are declared 4-byte aligned (a global dwordx4 access needs no more): a pixel of a channel slice of a wider tensor
// and a mirrored group at W % 4 != 0 straddle 16-byte boundaries and are still one instruction.
#include <algorithm>
#include "cnl_common.h"

#pragma clang fp contract(off)   // one add, one multiply

namespace cnl_flip {

constexpr int FLIP_THREADS = 256;
constexpr int FLIP_UNROLL = 4;           // items per lane per step: 8 loads of up to 16 bytes in flight before the first store
constexpr int FLIP_WG_PER_CU = 8;

typedef float f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4), aligned(4)));
static_assert(sizeof(cnl_flip_map) == 128, "cnl_flip_map of include/centernet_gfx950.h");

enum Mode { PIXEL4 = 0, ROW4 = 1, ELEMENT_C = 2, ELEMENT_X = 3 };

struct MergeArgs {
    cnl_flip_map map[3];
    unsigned items[3];
    int mode[3];
    int n_maps, N, H, W;
};

__device__ __forceinline__ float mean2(float a, float b) { return (a + b) * 0.5f; }

// One item of a map: where its operands and its result lie, and whether it is a vector of 4
struct Item {
    const float *a, *b;
    float* d;
    bool live, wide;
};

template <int MODE>
__device__ __forceinline__ Item locate(const cnl_flip_map& m, unsigned li, unsigned items, int H, int W) {
    Item it = {nullptr, nullptr, nullptr, li < items, false};
    if (!it.live) return it;
    const unsigned uH = (unsigned)H, uW = (unsigned)W, uC = (unsigned)m.C;
    unsigned n, c, y, x;
    if (MODE == PIXEL4) {
        const unsigned c4 = uC >> 2, pix = li / c4, row = pix / uW;
        c = (li - pix * c4) * 4u;
        x = pix - row * uW;
        n = row / uH;
        y = row - n * uH;
        it.wide = true;
    } else if (MODE == ROW4) {
        const unsigned groups = uW >> 2, per_row = groups + (uW & 3u), row = li / per_row, g = li - row * per_row, plane = row / uH;
        y = row - plane * uH;
        n = plane / uC;
        c = plane - n * uC;
        it.wide = g < groups;
        x = it.wide ? g * 4u : groups * 4u + (g - groups);
    } else if (MODE == ELEMENT_C) {
        const unsigned pix = li / uC, row = pix / uW;
        c = li - pix * uC;
        x = pix - row * uW;
        n = row / uH;
        y = row - n * uH;
    } else {
        const unsigned row = li / uW, plane = row / uH;
        x = li - row * uW;
        y = row - plane * uH;
        n = plane / uC;
        c = plane - n * uC;
    }
    // the mirrored operand: the swapped channel (box maps: 0 <-> 2; a PIXEL4 box item swaps components instead) at the mirrored column,
    // for a ROW4 vector the 4 columns that END there
    const unsigned pc = (MODE != PIXEL4 && m.swap_lr && !(c & 1u)) ? 2u - c : c;
    const unsigned bx = uW - 1u - x - ((MODE == ROW4 && it.wide) ? 3u : 0u);
    it.a = m.a + ((long long)n * m.a_sn + (long long)c * m.a_sc + (long long)y * m.a_sh + (long long)x * m.a_sw);
    it.b = m.b + ((long long)n * m.b_sn + (long long)pc * m.b_sc + (long long)y * m.b_sh + (long long)bx * m.b_sw);
    it.d = m.dst + ((long long)n * m.d_sn + (long long)c * m.d_sc + (long long)y * m.d_sh + (long long)x * m.d_sw);
    return it;
}

template <int MODE>
__device__ __forceinline__ void merge_map(const cnl_flip_map& m, unsigned items, int H, int W) {
    const unsigned step = gridDim.x * (unsigned)FLIP_THREADS;
    // (items < 2^31 and step * FLIP_UNROLL <= 2^23: the unsigned item numbers below cannot wrap)
    for (unsigned base = blockIdx.x * (unsigned)FLIP_THREADS + threadIdx.x; base < items; base += step * FLIP_UNROLL) {
        Item it[FLIP_UNROLL];
        f4 va[FLIP_UNROLL], vb[FLIP_UNROLL];
#pragma unroll
        for (int u = 0; u < FLIP_UNROLL; ++u) {
            it[u] = locate<MODE>(m, base + (unsigned)u * step, items, H, W);
            va[u] = vb[u] = (f4)(0.f);
            if (it[u].live) {
                if ((MODE == PIXEL4 || MODE == ROW4) && it[u].wide) {
                    va[u] = *reinterpret_cast<const f4*>(it[u].a);
                    vb[u] = *reinterpret_cast<const f4*>(it[u].b);
                } else {
                    va[u].x = *it[u].a;
                    vb[u].x = *it[u].b;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FLIP_UNROLL; ++u) {
            if (!it[u].live) continue;
            if ((MODE == PIXEL4 || MODE == ROW4) && it[u].wide) {
                f4 b = vb[u];
                if (MODE == ROW4) b = b.wzyx;
                else if (m.swap_lr) b = b.zyxw;
                f4 r;
                r.x = mean2(va[u].x, b.x);
                r.y = mean2(va[u].y, b.y);
                r.z = mean2(va[u].z, b.z);
                r.w = mean2(va[u].w, b.w);
                *reinterpret_cast<f4*>(it[u].d) = r;
            } else {
                *it[u].d = mean2(va[u].x, vb[u].x);
            }
        }
    }
}

__global__ __launch_bounds__(FLIP_THREADS) void flip_merge_kernel(MergeArgs q) {
    for (int i = 0; i < q.n_maps; ++i) {             // (uniform: the map's fields are scalar loads of the kernel arguments)
        const cnl_flip_map& m = q.map[i];
        switch (q.mode[i]) {
            case PIXEL4: merge_map<PIXEL4>(m, q.items[i], q.H, q.W); break;
            case ROW4: merge_map<ROW4>(m, q.items[i], q.H, q.W); break;
            case ELEMENT_C: merge_map<ELEMENT_C>(m, q.items[i], q.H, q.W); break;
            default: merge_map<ELEMENT_X>(m, q.items[i], q.H, q.W); break;
        }
    }
}

// An item is 4 bytes of one image row (row_bytes = W * C of them), written twice: as they are into the first half of dst, and gathered
// from the mirrored pixels into the second.  WORDS: rows start and end on 4-byte boundaries, so both stores are whole dwords.
template <int C, bool WORDS>
__global__ __launch_bounds__(FLIP_THREADS) void mirror_append_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                    unsigned items, unsigned per_row, unsigned row_bytes, unsigned half_bytes) {
    const unsigned step = gridDim.x * (unsigned)FLIP_THREADS;
    for (unsigned li = blockIdx.x * (unsigned)FLIP_THREADS + threadIdx.x; li < items; li += step) {
        const unsigned row = li / per_row, at = (li - row * per_row) * 4u;       // the item's first byte inside its row
        const unsigned char* s = src + (size_t)row * row_bytes;
        unsigned char* d = dst + (size_t)row * row_bytes + at;
        unsigned mirrored[4];
#pragma unroll
        for (unsigned e = 0; e < 4; ++e) {
            const unsigned byte = min(at + e, row_bytes - 1u), px = byte / (unsigned)C, ch = byte - px * (unsigned)C;
            mirrored[e] = s[row_bytes - (px + 1u) * (unsigned)C + ch];
        }
        if (WORDS) {
            *reinterpret_cast<unsigned*>(d) = *reinterpret_cast<const unsigned*>(s + at);
            *reinterpret_cast<unsigned*>(d + half_bytes) = mirrored[0] | mirrored[1] << 8 | mirrored[2] << 16 | mirrored[3] << 24;
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; ++e)
                if (at + e < row_bytes) {
                    d[e] = s[at + e];
                    d[half_bytes + e] = (unsigned char)mirrored[e];
                }
        }
    }
}

// workgroups of a grid-stride launch over `items` items at `per_wg` per workgroup and step: no more than FLIP_WG_PER_CU per CU
static int chip_grid(unsigned long long items, unsigned per_wg, unsigned* grid) {
    int dev = 0, n_cu = 0;
    CNL_HIP(hipGetDevice(&dev));
    if (int e = cnl::cu_count(dev, &n_cu)) return e;
    const unsigned long long wanted = (items + per_wg - 1) / per_wg, cap = (unsigned long long)std::max(n_cu, 1) * FLIP_WG_PER_CU;
    *grid = (unsigned)std::max(1ull, std::min(wanted, cap));
    return CNL_OK;
}

template <int C>
static int mirror_append(const uint8_t* src, uint8_t* dst, unsigned rows, unsigned row_bytes, unsigned half_bytes, void* stream) {
    const bool words = row_bytes % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    const unsigned per_row = (row_bytes + 3) / 4, items = rows * per_row;
    unsigned grid = 1;
    if (int e = chip_grid(items, FLIP_THREADS, &grid)) return e;
    if (words)
        hipLaunchKernelGGL((mirror_append_kernel<C, true>), dim3(grid), dim3(FLIP_THREADS), 0, (hipStream_t)stream, src, dst, items, per_row, row_bytes,
                           half_bytes);
    else
        hipLaunchKernelGGL((mirror_append_kernel<C, false>), dim3(grid), dim3(FLIP_THREADS), 0, (hipStream_t)stream, src, dst, items, per_row, row_bytes,
                           half_bytes);
    return cnl::check_launch("mirror_append_kernel");
}

}  // namespace cnl_flip

extern "C" int cnl_flip_merge_f32(const cnl_flip_map* maps, int32_t n_maps, int32_t N, int32_t H, int32_t W, void* stream) {
    using namespace cnl_flip;
    CNL_REQUIRE(n_maps >= 0 && n_maps <= 3, CNL_E_BAD_ARG, "cnl_flip_merge_f32: n_maps = %d outside 0..3", n_maps);
    CNL_REQUIRE(N >= 0 && H >= 0 && W >= 0, CNL_E_BAD_ARG, "cnl_flip_merge_f32: negative N, H or W");
    CNL_REQUIRE(n_maps == 0 || maps, CNL_E_BAD_ARG, "cnl_flip_merge_f32: null pointer (maps)");
    MergeArgs q = {};
    q.n_maps = n_maps;
    q.N = N;
    q.H = H;
    q.W = W;
    const unsigned long long pixels = (unsigned long long)N * (unsigned long long)H * (unsigned long long)W;
    unsigned long long most = 0;
    for (int i = 0; i < n_maps; ++i) {
        const cnl_flip_map& m = maps[i];
        CNL_REQUIRE(m.C >= 1, CNL_E_BAD_ARG, "cnl_flip_merge_f32: map %d: C = %d (at least one channel)", i, m.C);
        CNL_REQUIRE(!m.swap_lr || m.C == 4, CNL_E_BAD_ARG, "cnl_flip_merge_f32: map %d: swap_lr with C = %d (a box map has 4 channels)", i, m.C);
        CNL_REQUIRE(pixels * (unsigned long long)m.C <= 0x7fffffffull, CNL_E_BAD_ARG, "cnl_flip_merge_f32: map %d: N * C * H * W exceeds 2^31 - 1 elements", i);
        if (pixels == 0) continue;
        CNL_REQUIRE(m.a && m.b && m.dst, CNL_E_BAD_ARG, "cnl_flip_merge_f32: map %d: null pointer", i);
        CNL_REQUIRE((((uintptr_t)m.a | (uintptr_t)m.b | (uintptr_t)m.dst) & 3) == 0, CNL_E_BAD_ARG, "cnl_flip_merge_f32: map %d: pointers must be 4-byte aligned", i);
        q.map[i] = m;
        if (m.a_sc == 1 && m.b_sc == 1 && m.d_sc == 1 && m.C % 4 == 0) {
            q.mode[i] = PIXEL4;
            q.items[i] = (unsigned)(pixels * (unsigned)(m.C / 4));
        } else if (m.a_sw == 1 && m.b_sw == 1 && m.d_sw == 1) {
            q.mode[i] = ROW4;
            q.items[i] = (unsigned)((unsigned long long)N * m.C * H * (unsigned)(W / 4 + W % 4));
        } else {
            q.mode[i] = (m.d_sc < 0 ? -m.d_sc : m.d_sc) <= (m.d_sw < 0 ? -m.d_sw : m.d_sw) ? ELEMENT_C : ELEMENT_X;
            q.items[i] = (unsigned)(pixels * (unsigned)m.C);
        }
        most = std::max<unsigned long long>(most, q.items[i]);
    }
    if (most == 0) return CNL_OK;                    // nothing to merge: the pointers are not looked at
    unsigned grid = 1;
    if (int e = chip_grid(most, FLIP_THREADS * FLIP_UNROLL, &grid)) return e;
    hipLaunchKernelGGL(flip_merge_kernel, dim3(grid), dim3(FLIP_THREADS), 0, (hipStream_t)stream, q);
    return cnl::check_launch("flip_merge_kernel");
}

extern "C" int cnl_mirror_append_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    using namespace cnl_flip;
    CNL_REQUIRE(N >= 0 && H >= 0 && W >= 0, CNL_E_BAD_ARG, "cnl_mirror_append_u8: negative N, H or W");
    CNL_REQUIRE(C >= 1 && C <= 4, CNL_E_BAD_ARG, "cnl_mirror_append_u8: C = %d outside 1..4", C);
    const unsigned long long half = (unsigned long long)N * (unsigned long long)H * (unsigned long long)W * (unsigned long long)C;
    CNL_REQUIRE(2 * half <= 0x7fffffffull, CNL_E_BAD_ARG, "cnl_mirror_append_u8: the doubled batch exceeds 2^31 - 1 bytes");
    if (half == 0) return CNL_OK;                    // no pixels: a no-op whose pointers are not looked at
    CNL_REQUIRE(src && dst, CNL_E_BAD_ARG, "cnl_mirror_append_u8: null pointer");
    const unsigned rows = (unsigned)N * (unsigned)H, row_bytes = (unsigned)W * (unsigned)C;
    switch (C) {
        case 1: return mirror_append<1>(src, dst, rows, row_bytes, (unsigned)half, stream);
        case 2: return mirror_append<2>(src, dst, rows, row_bytes, (unsigned)half, stream);
        case 3: return mirror_append<3>(src, dst, rows, row_bytes, (unsigned)half, stream);
        default: return mirror_append<4>(src, dst, rows, row_bytes, (unsigned)half, stream);
    }
}
