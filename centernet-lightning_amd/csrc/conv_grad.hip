// Convolution backward for the heads (include/centernet_gfx950.h, "Convolution gradients"): the ReLU mask + bias gradient, the weight
// gradient of a 3x3 / 1x1 stride-1 conv and the input gradient of a 1x1 conv.  fp32 only: every product of the weight gradient runs on the fp32
// matrix cores (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain), the 1x1 input gradient is an explicit fmaf chain on the vector ALU.
// No fp16 split here: its promise is "inputs within 1e4 of the image maximum", and a loss gradient map (a focal-loss peak beside far negatives)
// spans many more decades.  No atomics, no memset: partial results go to a workspace and a second launch adds them in a fixed order.
#include "cnl_common.h"

namespace cnl_grad {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr long long ADDRESS_LIMIT = 0xF0000000ll - (1 << 24);      // bytes one tensor may span (the engine's limit: 32-bit pixel indices stay exact)

// ---- weight gradient ---------------------------------------------------------------------------------------------------------------------
// dW[co][tap][ci] = sum over pixels of dz[pixel][co] * x[pixel + tap][ci]: a GEMM with M = Cout, N = taps * Cin, K = N * H * W.
// A workgroup (4 waves) owns WG_CO couts x all taps x WG_CI input channels for ONE slice of the image rows; wave w owns the 32 couts
// [32 w, 32 w + 32) of the tile, one 32 x 32 accumulator per tap.  Per chunk of WG_TW pixels of one row it stages dz[WG_TW][WG_CO] and the x rows
// with their one-pixel halo ([KS][WG_TW + 2][WG_CI], zero outside the image) in LDS: every x element staged serves all taps.  A matrix
// instruction takes two neighbouring pixels (k = 0 / 1 in the two lane halves): A = dz[pixel][co], B = x[pixel + tap][ci].
constexpr int WG_CO = 128, WG_CI = 32, WG_TW = 64;
constexpr int WG_TARGET = 1024;      // workgroups a launch aims for (4 per CU of a 256-CU chip: two resident, two waiting)
constexpr int WG_MIN_PIX = 512;      // a slice holds at least this many pixels (bounds the workspace of small maps)

struct Geom {
    int taps, tiles, ci_slices;
    long long rows, rows_per_slice, slices;
};

// The slice function of the header: from the layer shape and N, H, W alone.
static bool wgrad_geom(int N, int H, int W, int Cin, int Cout, int KH, int KW, Geom* g) {
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return false;
    if (!((KH == 3 && KW == 3) || (KH == 1 && KW == 1)) || Cin % 32) return false;
    g->taps = KH * KW;
    g->ci_slices = Cin / WG_CI;
    const long long tiles = (long long)((Cout + WG_CO - 1) / WG_CO) * g->ci_slices;
    if (tiles > (1 << 24)) return false;
    g->tiles = (int)tiles;
    g->rows = (long long)N * H;
    const long long s0 = (WG_TARGET + tiles - 1) / tiles;
    long long rps = (g->rows + s0 - 1) / s0;
    const long long floor_rows = (WG_MIN_PIX + W - 1) / W;
    if (rps < floor_rows) rps = floor_rows;
    if (rps > g->rows) rps = g->rows;
    g->rows_per_slice = rps;
    g->slices = (g->rows + rps - 1) / rps;
    return true;
}

template <int KS>
__global__ __launch_bounds__(THREADS, 2) void wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ ws, int H, int W,
                                                        int Cin, int Cout, int ldx, int lddz, long long rows, long long rps, int ci_slices, int tiles) {
    constexpr int TAPS = KS * KS, PAD = KS / 2, XW = WG_TW + 2 * PAD;
    __shared__ __attribute__((aligned(16))) float dzs[WG_TW * WG_CO];          // [pixel][co]
    __shared__ __attribute__((aligned(16))) float xs[KS * XW * WG_CI];         // [ky][pixel + halo][ci]
    const unsigned id = cnl::xcd_remap(blockIdx.x, gridDim.x);                 // the tiles of one slice read the same rows: keep them on one XCD
    const long long slice = id / (unsigned)tiles;
    const int tile = (int)(id % (unsigned)tiles);
    const int co0 = (tile / ci_slices) * WG_CO, ci0 = (tile % ci_slices) * WG_CI;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kp = lane >> 5;
    const int cob = wave * 32;
    const bool active = co0 + cob < Cout;                                      // wave-uniform: a wave whose 32 couts lie past Cout only stages

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const long long r0 = slice * rps;
    const long long r1 = r0 + rps < rows ? r0 + rps : rows;
    for (long long r = r0; r < r1; ++r) {
        const int oy = (int)(r % H);
        const long long img_row0 = r - oy;                                     // n * H
        for (int ox0 = 0; ox0 < W; ox0 += WG_TW) {
#pragma unroll
            for (int i = tid; i < WG_TW * (WG_CO / 4); i += THREADS) {
                const int px = i / (WG_CO / 4), c4 = (i % (WG_CO / 4)) * 4;
                const int ox = ox0 + px, co = co0 + c4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ox < W && co < Cout) {
                    // an aligned 16-byte word whose first float is a declared channel: the floats past Cout (other channels of a wider buffer) are dropped
                    v = *reinterpret_cast<const f32x4*>(dz + ((r * W + ox) * (long long)lddz + co));
                    if (co + 1 >= Cout) v[1] = 0.f;
                    if (co + 2 >= Cout) v[2] = 0.f;
                    if (co + 3 >= Cout) v[3] = 0.f;
                }
                *reinterpret_cast<f32x4*>(&dzs[px * WG_CO + c4]) = v;
            }
            for (int i = tid; i < KS * XW * (WG_CI / 4); i += THREADS) {
                const int c4 = (i % (WG_CI / 4)) * 4, t = i / (WG_CI / 4);
                const int px = t % XW, ky = t / XW;
                const int iy = oy + ky - PAD, ix = ox0 + px - PAD;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (iy >= 0 && iy < H && ix >= 0 && ix < W)
                    v = *reinterpret_cast<const f32x4*>(x + (((img_row0 + iy) * W + ix) * (long long)ldx + ci0 + c4));
                *reinterpret_cast<f32x4*>(&xs[(ky * XW + px) * WG_CI + c4]) = v;
            }
            __syncthreads();
            if (active) {
                const int valid = W - ox0 < WG_TW ? W - ox0 : WG_TW;
                const int pairs = (valid + 1) / 2;                             // an odd tail pairs with a pixel whose dz was staged as zero
                for (int pp = 0; pp < pairs; ++pp) {
                    const int k = 2 * pp + kp;
                    const float a = dzs[k * WG_CO + cob + l31];
#pragma unroll
                    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                        for (int kx = 0; kx < KS; ++kx) {
                            const float b = xs[(ky * XW + k + kx) * WG_CI + l31];
                            acc[ky * KS + kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[ky * KS + kx], 0, 0, 0);
                        }
                }
            }
            __syncthreads();
        }
    }
    if (!active) return;
    // partial tile -> ws[slice][co][tap][ci]; accumulator register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cob + (r & 3) + 8 * (r >> 2) + 4 * kp;
            if (co < Cout) ws[((slice * Cout + co) * TAPS + t) * (long long)Cin + ci0 + l31] = acc[t][r];
        }
}

// dW = slice 0 + slice 1 + ... in slice order
__global__ __launch_bounds__(THREADS) void wgrad_reduce_kernel(const f32x4* __restrict__ ws, f32x4* __restrict__ dw, long long quads, long long slices) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= quads) return;
    f32x4 s = ws[i];
    for (long long sl = 1; sl < slices; ++sl) s += ws[sl * quads + i];
    dw[i] = s;
}

// ---- ReLU mask + bias gradient --------------------------------------------------------------------------------------------------------------
// A workgroup owns RG_PIX consecutive pixels.  cpt = min(256, C rounded up to a power of two) threads cover the channels of a pixel, the 256 / cpt
// "pixel lanes" walk the workgroup's pixels with stride 256 / cpt; a lane's sum runs in pixel order, the lanes are added in lane order.
constexpr int RG_PIX = 256;

__global__ __launch_bounds__(THREADS) void relu_grad_kernel(const float* __restrict__ dy, long long sn, long long sc, long long sh, long long sw,
                                                            const float* __restrict__ y, int ldy, int C, int H, int W, long long P, float* __restrict__ dz,
                                                            int lddz, float* __restrict__ part, int cpt) {
    __shared__ float red[THREADS];
    const int tid = threadIdx.x;
    const int pl = THREADS / cpt, c0 = tid % cpt, lp = tid / cpt;
    const long long p0 = (long long)blockIdx.x * RG_PIX;
    const int npx = (int)(P - p0 < RG_PIX ? P - p0 : RG_PIX);
    for (int cb = 0; cb < C; cb += cpt) {
        const int c = cb + c0;
        float acc = 0.f;
        if (c < C) {
            for (int j = lp; j < npx; j += pl) {
                const unsigned p = (unsigned)(p0 + j);                         // P <= 2^30 (the address limit)
                const unsigned wi = p % (unsigned)W, t = p / (unsigned)W;
                const unsigned hi = t % (unsigned)H, n = t / (unsigned)H;
                float g = dy[(long long)n * sn + (long long)c * sc + (long long)hi * sh + (long long)wi * sw];
                if (y != nullptr && !(y[(long long)p * ldy + c] > 0.f)) g = 0.f;
                dz[(long long)p * lddz + c] = g;
                acc += g;
            }
        }
        if (part != nullptr) {
            if (pl == 1) {
                if (c < C) part[(long long)blockIdx.x * C + c] = acc;
            } else {
                red[tid] = acc;
                __syncthreads();
                if (lp == 0 && c < C) {
                    float s = red[c0];
                    for (int j = 1; j < pl; ++j) s += red[j * cpt + c0];
                    part[(long long)blockIdx.x * C + c] = s;
                }
                __syncthreads();
            }
        }
    }
}

// dbias[c] = the workgroups' partial sums added in workgroup order, in float64, rounded once
__global__ __launch_bounds__(THREADS) void bias_finish_kernel(const float* __restrict__ part, long long blocks, int C, float* __restrict__ dbias) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (long long b = 0; b < blocks; ++b) s += (double)part[b * C + c];
    dbias[c] = (float)s;
}

// ---- 1x1 input gradient ----------------------------------------------------------------------------------------------------------------------
// dx[p][ci] = fmaf chain over co = 0, 1, ... of dz[p][co] * w[co][ci].  A workgroup owns DG_PIX pixels; per block of 128 input channels a thread
// owns 8 pixels x 4 channels; dz is staged [co][pixel] in LDS in chunks of DG_CO couts.
constexpr int DG_PIX = 64, DG_CO = 64, DG_LD = 68;

__global__ __launch_bounds__(THREADS) void dgrad1x1_kernel(const float* __restrict__ dz, int lddz, const float* __restrict__ w, float* __restrict__ dx,
                                                           int lddx, long long P, int Cin, int Cout) {
    __shared__ __attribute__((aligned(16))) float dzs[DG_CO * DG_LD];
    const int tid = threadIdx.x;
    const int g = tid & 31, pg = tid >> 5;
    const long long p0 = (long long)blockIdx.x * DG_PIX;
    const int npx = (int)(P - p0 < DG_PIX ? P - p0 : DG_PIX);
    for (int cib = 0; cib < Cin; cib += 128) {
        const int ci = cib + g * 4;
        f32x4 acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int cc = 0; cc < Cout; cc += DG_CO) {
            const int nco = Cout - cc < DG_CO ? Cout - cc : DG_CO;
#pragma unroll
            for (int i = tid; i < DG_PIX * (DG_CO / 4); i += THREADS) {
                const int c4 = (i % (DG_CO / 4)) * 4, px = i / (DG_CO / 4);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (px < npx && c4 < nco) {
                    v = *reinterpret_cast<const f32x4*>(dz + ((p0 + px) * (long long)lddz + cc + c4));     // aligned word, first float declared
                    if (c4 + 1 >= nco) v[1] = 0.f;
                    if (c4 + 2 >= nco) v[2] = 0.f;
                    if (c4 + 3 >= nco) v[3] = 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) dzs[(c4 + e) * DG_LD + px] = v[e];
            }
            __syncthreads();
            if (ci < Cin) {
                for (int co = 0; co < nco; ++co) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + ((long long)(cc + co) * Cin + ci));
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(&dzs[co * DG_LD + pg * 8]);
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(&dzs[co * DG_LD + pg * 8 + 4]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc[j][e] = __builtin_fmaf(a0[j], wv[e], acc[j][e]);
                            acc[j + 4][e] = __builtin_fmaf(a1[j], wv[e], acc[j + 4][e]);
                        }
                }
            }
            __syncthreads();
        }
        if (ci < Cin) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int px = pg * 8 + j;
                if (px < npx) *reinterpret_cast<f32x4*>(dx + ((p0 + px) * (long long)lddx + ci)) = acc[j];
            }
        }
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace cnl_grad

extern "C" int64_t cnl_conv_wgrad_slices(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW) {
    cnl_grad::Geom g;
    return cnl_grad::wgrad_geom(N, H, W, Cin, Cout, KH, KW, &g) ? (int64_t)g.slices : 0;
}

extern "C" size_t cnl_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW) {
    cnl_grad::Geom g;
    if (!cnl_grad::wgrad_geom(N, H, W, Cin, Cout, KH, KW, &g)) return 0;
    return (size_t)g.slices * (size_t)Cout * (size_t)g.taps * (size_t)Cin * sizeof(float);
}

extern "C" int64_t cnl_conv_wgrad_terms(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW) {
    cnl_grad::Geom g;
    if (!cnl_grad::wgrad_geom(N, H, W, Cin, Cout, KH, KW, &g)) return 0;
    return (int64_t)(g.rows_per_slice * W + g.slices);
}

extern "C" int cnl_conv_wgrad_nhwc_f32(const float* x, int32_t ldx, const float* dz, int32_t lddz, float* dw, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                       int32_t Cout, int32_t KH, int32_t KW, int32_t pad, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace cnl_grad;
    CNL_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, CNL_E_BAD_ARG, "cnl_conv_wgrad_nhwc_f32: non-positive dimension (N %d, H %d, W %d, Cin %d, Cout %d)",
                N, H, W, Cin, Cout);
    CNL_REQUIRE(x && dz && dw, CNL_E_BAD_ARG, "cnl_conv_wgrad_nhwc_f32: null pointer (x, dz or dw)");
    CNL_REQUIRE((KH == 3 && KW == 3 && pad == 1) || (KH == 1 && KW == 1 && pad == 0), CNL_E_UNSUPPORTED,
                "cnl_conv_wgrad_nhwc_f32: kernel %d x %d with pad %d (3 x 3 / pad 1 and 1 x 1 / pad 0, stride 1)", KH, KW, pad);
    CNL_REQUIRE(Cin % 32 == 0, CNL_E_UNSUPPORTED, "cnl_conv_wgrad_nhwc_f32: Cin = %d is not a multiple of 32", Cin);
    CNL_REQUIRE(ldx >= Cin && ldx % 4 == 0 && aligned16(x), CNL_E_BAD_ARG, "cnl_conv_wgrad_nhwc_f32: x needs ldx >= Cin, ldx %% 4 == 0 and 16-byte alignment (ldx %d, Cin %d)",
                ldx, Cin);
    CNL_REQUIRE(lddz >= Cout && lddz % 4 == 0 && aligned16(dz), CNL_E_BAD_ARG,
                "cnl_conv_wgrad_nhwc_f32: dz needs lddz >= Cout, lddz %% 4 == 0 and 16-byte alignment (lddz %d, Cout %d)", lddz, Cout);
    CNL_REQUIRE(aligned16(dw), CNL_E_BAD_ARG, "cnl_conv_wgrad_nhwc_f32: dw must be 16-byte aligned");
    const long long P = (long long)N * H * W;
    CNL_REQUIRE(P * ldx * 4 <= ADDRESS_LIMIT && P * lddz * 4 <= ADDRESS_LIMIT, CNL_E_UNSUPPORTED,
                "cnl_conv_wgrad_nhwc_f32: a tensor of %lld pixels spans more than the 4 GiB addressing (split the batch)", P);
    Geom g;
    CNL_REQUIRE(wgrad_geom(N, H, W, Cin, Cout, KH, KW, &g), CNL_E_UNSUPPORTED, "cnl_conv_wgrad_nhwc_f32: shape outside the slice function");
    const long long elems = (long long)Cout * g.taps * Cin;
    const size_t need = (size_t)g.slices * (size_t)elems * sizeof(float);
    CNL_REQUIRE(g.slices * (long long)g.tiles <= 0x7fffffffll, CNL_E_UNSUPPORTED, "cnl_conv_wgrad_nhwc_f32: too many workgroups");
    CNL_REQUIRE(workspace && workspace_bytes >= need, CNL_E_WORKSPACE, "cnl_conv_wgrad_nhwc_f32: workspace of %zu bytes, needs %zu (cnl_conv_wgrad_workspace_bytes)",
                workspace ? workspace_bytes : (size_t)0, need);
    CNL_REQUIRE(aligned16(workspace), CNL_E_BAD_ARG, "cnl_conv_wgrad_nhwc_f32: workspace must be 16-byte aligned");
    float* ws = static_cast<float*>(workspace);
    const unsigned grid = (unsigned)(g.slices * g.tiles);
    if (KH == 3)
        hipLaunchKernelGGL((wgrad_kernel<3>), dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, x, dz, ws, H, W, Cin, Cout, ldx, lddz, g.rows, g.rows_per_slice,
                           g.ci_slices, g.tiles);
    else
        hipLaunchKernelGGL((wgrad_kernel<1>), dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, x, dz, ws, H, W, Cin, Cout, ldx, lddz, g.rows, g.rows_per_slice,
                           g.ci_slices, g.tiles);
    if (int e = cnl::check_launch("wgrad_kernel")) return e;
    const long long quads = elems / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((quads + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(ws), reinterpret_cast<f32x4*>(dw), quads, g.slices);
    return cnl::check_launch("wgrad_reduce_kernel");
}

extern "C" size_t cnl_relu_grad_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return 0;
    const long long P = (long long)N * H * W;
    return (size_t)((P + cnl_grad::RG_PIX - 1) / cnl_grad::RG_PIX) * (size_t)C * sizeof(float);
}

extern "C" int64_t cnl_relu_grad_terms(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return 0;
    return cnl_grad::RG_PIX + 1;
}

extern "C" int cnl_relu_grad_f32(const float* dy, int64_t dy_sn, int64_t dy_sc, int64_t dy_sh, int64_t dy_sw, const float* y, int32_t ldy, int32_t N, int32_t C,
                                 int32_t H, int32_t W, float* dz, int32_t lddz, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace cnl_grad;
    CNL_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, CNL_E_BAD_ARG, "cnl_relu_grad_f32: non-positive dimension (N %d, C %d, H %d, W %d)", N, C, H, W);
    CNL_REQUIRE(dy && dz, CNL_E_BAD_ARG, "cnl_relu_grad_f32: null pointer (dy or dz)");
    CNL_REQUIRE(dy_sn >= 0 && dy_sc >= 0 && dy_sh >= 0 && dy_sw >= 0, CNL_E_BAD_ARG, "cnl_relu_grad_f32: negative dy stride");
    CNL_REQUIRE(lddz >= C && lddz % 4 == 0 && aligned16(dz), CNL_E_BAD_ARG, "cnl_relu_grad_f32: dz needs lddz >= C, lddz %% 4 == 0 and 16-byte alignment (lddz %d, C %d)",
                lddz, C);
    CNL_REQUIRE(!y || ldy >= C, CNL_E_BAD_ARG, "cnl_relu_grad_f32: ldy = %d below C = %d", ldy, C);
    CNL_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dbias)) & 3) == 0, CNL_E_BAD_ARG,
                "cnl_relu_grad_f32: dy, y and dbias must be 4-byte aligned");
    const long long P = (long long)N * H * W;
    CNL_REQUIRE(P * lddz * 4 <= ADDRESS_LIMIT && (!y || P * ldy * 4 <= ADDRESS_LIMIT), CNL_E_UNSUPPORTED,
                "cnl_relu_grad_f32: a tensor of %lld pixels spans more than the 4 GiB addressing (split the batch)", P);
    const long long blocks = (P + RG_PIX - 1) / RG_PIX;
    float* part = nullptr;
    if (dbias) {
        const size_t need = (size_t)blocks * (size_t)C * sizeof(float);
        CNL_REQUIRE(workspace && workspace_bytes >= need, CNL_E_WORKSPACE, "cnl_relu_grad_f32: workspace of %zu bytes, needs %zu (cnl_relu_grad_workspace_bytes)",
                    workspace ? workspace_bytes : (size_t)0, need);
        CNL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, CNL_E_BAD_ARG, "cnl_relu_grad_f32: workspace must be 4-byte aligned");
        part = static_cast<float*>(workspace);
    }
    int cpt = 1;
    while (cpt < C && cpt < THREADS) cpt *= 2;
    hipLaunchKernelGGL(relu_grad_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, dy, (long long)dy_sn, (long long)dy_sc, (long long)dy_sh,
                       (long long)dy_sw, y, ldy, C, H, W, P, dz, lddz, part, cpt);
    if (int e = cnl::check_launch("relu_grad_kernel")) return e;
    if (!dbias) return CNL_OK;
    hipLaunchKernelGGL(bias_finish_kernel, dim3((unsigned)((C + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, part, blocks, C, dbias);
    return cnl::check_launch("bias_finish_kernel");
}

extern "C" int cnl_conv1x1_dgrad_nhwc_f32(const float* dz, int32_t lddz, const float* w, float* dx, int32_t lddx, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                          int32_t Cout, void* stream) {
    using namespace cnl_grad;
    CNL_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, CNL_E_BAD_ARG, "cnl_conv1x1_dgrad_nhwc_f32: non-positive dimension (N %d, H %d, W %d, Cin %d, Cout %d)",
                N, H, W, Cin, Cout);
    CNL_REQUIRE(dz && w && dx, CNL_E_BAD_ARG, "cnl_conv1x1_dgrad_nhwc_f32: null pointer (dz, w or dx)");
    CNL_REQUIRE(Cin % 32 == 0, CNL_E_UNSUPPORTED, "cnl_conv1x1_dgrad_nhwc_f32: Cin = %d is not a multiple of 32", Cin);
    CNL_REQUIRE(lddz >= Cout && lddz % 4 == 0 && aligned16(dz), CNL_E_BAD_ARG,
                "cnl_conv1x1_dgrad_nhwc_f32: dz needs lddz >= Cout, lddz %% 4 == 0 and 16-byte alignment (lddz %d, Cout %d)", lddz, Cout);
    CNL_REQUIRE(lddx >= Cin && lddx % 4 == 0 && aligned16(dx), CNL_E_BAD_ARG,
                "cnl_conv1x1_dgrad_nhwc_f32: dx needs lddx >= Cin, lddx %% 4 == 0 and 16-byte alignment (lddx %d, Cin %d)", lddx, Cin);
    CNL_REQUIRE(aligned16(w), CNL_E_BAD_ARG, "cnl_conv1x1_dgrad_nhwc_f32: w must be 16-byte aligned");
    const long long P = (long long)N * H * W;
    CNL_REQUIRE(P * lddz * 4 <= ADDRESS_LIMIT && P * lddx * 4 <= ADDRESS_LIMIT, CNL_E_UNSUPPORTED,
                "cnl_conv1x1_dgrad_nhwc_f32: a tensor of %lld pixels spans more than the 4 GiB addressing (split the batch)", P);
    hipLaunchKernelGGL(dgrad1x1_kernel, dim3((unsigned)((P + DG_PIX - 1) / DG_PIX)), dim3(THREADS), 0, (hipStream_t)stream, dz, lddz, w, dx, lddx, P, Cin, Cout);
    return cnl::check_launch("dgrad1x1_kernel");
}
