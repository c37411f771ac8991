// pointwise.hip — the 1x1 convolutions of the ResNet-50 / 101 bottleneck blocks as one GEMM [N*Ho*Wo, K] x [K, Cout] over NHWC rows
// (torchvision Bottleneck.conv1 / conv3 / downsample), on the three-term fp16 split of conv_f16x2.hip.
//
// Single-source form: y = act(x1 W + b (+ residual)).  Two-source form: y = act(x1 W3 + x2[::s, ::s] Wds + b3 + bds) — a stage's conv3 and its
// downsample in one launch: the K loop runs over the 32-channel chunks of x1 and then over those of x2 read at stride s (1 or 2), the weights
// are [W3 | Wds] concatenated along K and pre-split once at weight load (cnl_conv_split_weights_f32 with Cin = K1 + K2), the biases are summed.
// The downsample's output never reaches memory.
//
// Arithmetic: row m (an output pixel of image n) is scaled by ONE power of two S_n from max(max |x1[n]|, max |x2[n]|) (the x_absmax hints of
// both sources), the weights by S_w (pre-split); x S = hi + lo (RN16 / RZ16 of the exact residual), and x w S_n S_w is accumulated in fp32 as
// hi lo' + lo hi' + hi hi' on v_mfma_f32_32x32x16_f16; the epilogue multiplies by 1 / (S_n S_w).  A row's scale depends on its own image only:
// a shard gives the same bits as the full batch.  The error bound of the shared scale is in DESIGN.md §11.
//
// Structure: conv_f16x2.hip's with the tap loop gone — A rows (pixels) and B rows (pre-split weight rows) of a 32-channel chunk are staged by
// LDS-DMA into two stages (the DMA of chunk kt + 1 runs under the matrix work of chunk kt), one barrier per chunk, 4 waves, two workgroups
// per CU.  The epilogue adds bias (+ residual), clamps, stores NHWC and folds max |y| per image into y_absmax with vector atomics.
#include "conv_args.h"

namespace cnl_pw {
using namespace cnl_conv;


struct PwArgs {
    const float* x1;
    const float* x2;          // null: single source
    const float* wsplit;      // [Cout][K] scaled fp16 pieces in the B-row layout of conv_f16x2.hip
    const float* wscale;      // S_w
    const float* bias;
    const float* res;
    float* y;
    const float* xmax1;
    const float* xmax2;
    unsigned* ymax;
    int N, Ho, Wo, M, Cout;
    int KT1, KT, K;           // chunks of x1, chunks in all, K = 32 KT
    int ldx1, ldx2, ldy, ldr;
    int H2, W2, s2;
    unsigned x1_bytes, x2_bytes, w_bytes, y_bytes, r_bytes;
    unsigned flags;
    int tiles_n, tiles;
    unsigned mg_hw, sh_hw, mg_w, sh_w;
};


template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256, 2) void pointwise_kernel(const PwArgs a) {
    using C = Cfg<WM, WN, TM, TN>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sInv = reinterpret_cast<float*>(smem + C::LDS_BYTES);      // [BM] 1 / (S_row S_w)
    float* sScl = sInv + C::BM;                                       // [BM] S_row
    int* sImg = reinterpret_cast<int*>(sScl + C::BM);                 // [BM] image of the row (-1 beyond M)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int hi = lane >> 5;

    const unsigned tile = cnl::xcd_remap(blockIdx.x, (unsigned)a.tiles);
    const int n_tile = tile % a.tiles_n;
    const int m_tile = tile / a.tiles_n;
    const int m0 = m_tile * C::BM;
    const int n0 = n_tile * C::BN;

    // ---- per-lane staging offsets: row r of the A tile is pixel m0 + r of x1, and pixel (n, s oy, s ox) of x2 ----
    const int lrow = lane >> 3;
    const int pslot = lane & 7;
    unsigned a_off1[C::A_INSTR], a_off2[C::A_INSTR];
#pragma unroll
    for (int j = 0; j < C::A_INSTR; ++j) {
        const int r = (j * C::NW + wave) * 8 + lrow;
        const int m = m0 + r;
        const int q = (pslot ^ ((r >> 1) & 7)) * 4;
        const bool ok = m < a.M;
        a_off1[j] = ok ? (unsigned)(((long long)m * a.ldx1 + q) * 4) : OOB;
        const unsigned n = fast_div((unsigned)m, a.mg_hw, a.sh_hw);
        const unsigned rem = (unsigned)m - n * (unsigned)(a.Ho * a.Wo);
        const unsigned oy = fast_div(rem, a.mg_w, a.sh_w);
        const unsigned ox = rem - oy * (unsigned)a.Wo;
        const long long p2 = ((long long)n * a.H2 + (long long)oy * a.s2) * a.W2 + (long long)ox * a.s2;
        a_off2[j] = (ok && a.x2) ? (unsigned)((p2 * a.ldx2 + q) * 4) : OOB;
    }
    unsigned b_off[C::B_INSTR];
#pragma unroll
    for (int j = 0; j < C::B_INSTR; ++j) {
        const int r = (j * C::NW + wave) * 8 + lrow;
        const int q = (pslot ^ ((r >> 1) & 7)) * 4;
        b_off[j] = (n0 + r) < a.Cout ? (unsigned)(((n0 + r) * a.K + q) * 4) : OOB;
    }
    // chunk kt into stage st: x1 for kt < KT1, x2 after (the branch is uniform)
#define PW_ISSUE(st_, kt_)                                                                                            \
    do {                                                                                                              \
        char* sA_ = smem + (st_) * C::STAGE_BYTES;                                                                    \
        char* sB_ = sA_ + C::BM * 128;                                                                                \
        if ((kt_) < a.KT1) {                                                                                          \
            _Pragma("unroll") for (int j = 0; j < C::A_INSTR; ++j)                                                    \
                dma16(a.x1, a.x1_bytes, sA_ + (j * C::NW + wave) * 1024, a_off1[j], (unsigned)((kt_) * 128));         \
        } else {                                                                                                      \
            _Pragma("unroll") for (int j = 0; j < C::A_INSTR; ++j)                                                    \
                dma16(a.x2, a.x2_bytes, sA_ + (j * C::NW + wave) * 1024, a_off2[j], (unsigned)(((kt_) - a.KT1) * 128)); \
        }                                                                                                             \
        _Pragma("unroll") for (int j = 0; j < C::B_INSTR; ++j)                                                        \
            dma16(a.wsplit, a.w_bytes, sB_ + (j * C::NW + wave) * 1024, b_off[j], (unsigned)((kt_) * 128));           \
    } while (0)
    PW_ISSUE(0, 0);          // first chunk in flight before anything else

    // ---- scales: one per row of the tile (its image's, over both sources), one for the weights ----
    const float Sw = *a.wscale;
    for (int r = threadIdx.x; r < C::BM; r += C::THREADS) {
        const int m = m0 + r;
        const unsigned n = fast_div((unsigned)m, a.mg_hw, a.sh_hw);
        const bool ok = m < a.M;
        float mx = 0.f;
        if (ok) {
            mx = a.xmax1[n * AMS];
            if (a.x2) mx = fmaxf(mx, a.xmax2[n * AMS]);
        }
        const float S = ok ? pow2_scale(mx) : 1.f;
        sScl[r] = S;
        sInv[r] = 1.f / (S * Sw);
        sImg[r] = ok ? (int)n : -1;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int swz = (lane >> 1) & 7;
    const int a_row_byte = (wm * TM * 32 + (lane & 31)) * 128;
    const int b_row_byte = C::BM * 128 + (wn * TN * 32 + (lane & 31)) * 128;
    f32x4 ra[2][TM], rb[2][TN];
    u32x4 ah[TM], al[TM], bh[TN], bl[TN];
    float sA[TM];

#define PW_READ(stage_ptr_, g_)                                                                                       \
    do {                                                                                                              \
        _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) {                                                            \
            const int sb_ = (((2 * (2 * (g_) + q_) + hi) ^ swz) << 4);                                                \
            const int sbb_ = (((2 * (2 * (g_) + hi) + q_) ^ swz) << 4);                                               \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) ra[q_][i] = lds_read16((stage_ptr_) + a_row_byte + i * 32 * 128 + sb_); \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) rb[q_][j] = lds_read16((stage_ptr_) + b_row_byte + j * 32 * 128 + sbb_); \
        }                                                                                                             \
    } while (0)
#define PW_SPLIT()                                                                                                    \
    do {                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) split8(ra[0][i], ra[1][i], sA[i], ah[i], al[i]);               \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                              \
            bh[j] = __builtin_bit_cast(u32x4, rb[0][j]);                                                              \
            bl[j] = __builtin_bit_cast(u32x4, rb[1][j]);                                                              \
        }                                                                                                             \
    } while (0)
#define PW_MFMA()                                                                                                     \
    do {                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(ah[i], bl[j], acc[i][j]);               \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(al[i], bh[j], acc[i][j]);               \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(ah[i], bh[j], acc[i][j]);               \
    } while (0)

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // chunk 0 landed (this wave) ...
    __syncthreads();                                    // ... and everyone's, and the scale tables are written
#pragma unroll
    for (int i = 0; i < TM; ++i) sA[i] = sScl[(wm * TM + i) * 32 + (lane & 31)];
    if (a.KT > 1) PW_ISSUE(1, 1);
    PW_READ(smem, 0);
    // One chunk = two 16-channel groups; the barrier of chunk kt sits between them: (a) every wave has its group-1 fragments of chunk kt in
    // registers -> the stage may be refilled with chunk kt + 2, (b) every wave's DMA of chunk kt + 1 has landed -> it may be read.
    for (int kt = 0; kt < a.KT; ++kt) {
        const char* sS = smem + (kt & 1) * C::STAGE_BYTES;
        const char* sN = smem + ((kt + 1) & 1) * C::STAGE_BYTES;
        PW_SPLIT();
        PW_READ(sS, 1);
        PW_MFMA();
        PW_SPLIT();
        if (kt + 1 < a.KT) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 2 < a.KT) PW_ISSUE(kt & 1, kt + 2);
            PW_READ(sN, 0);
        }
        PW_MFMA();
    }
#undef PW_ISSUE
#undef PW_READ
#undef PW_SPLIT
#undef PW_MFMA

    // ---- epilogue: row scale back, + bias (+ residual) -> clamp -> NHWC store; max |y| per image ----
    const float lo = (a.flags & CNL_RELU) ? 0.f : -__builtin_inff();
    const int img0 = sImg[0];
    float omax = 0.f, omax1 = 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
        const bool col_ok = col < a.Cout;
        const float bv = col_ok ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rl = (wm * TM + i) * 32 + 4 * hi;
            const int mb = m0 + rl;
            const unsigned y_voff = (unsigned)(((long long)mb * a.ldy + col) * 4);
            const unsigned r_voff = (unsigned)(((long long)mb * a.ldr + col) * 4);
            float v[16];
            bool ok[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                ok[r] = col_ok && mb + ro < a.M;
                v[r] = acc[i][j][r] * sInv[rl + ro] + bv;
            }
            if (a.res) {
                float rv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    rv[r] = buf_load(a.res, a.r_bytes, ok[r] ? r_voff : OOB, (unsigned)(((r & 3) + 8 * (r >> 2)) * a.ldr * 4));
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += rv[r];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = fmaxf(v[r], lo);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                buf_store(v[r], a.y, a.y_bytes, ok[r] ? y_voff : OOB, (unsigned)(((r & 3) + 8 * (r >> 2)) * a.ldy * 4));
            if (a.ymax) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float av = ok[r] ? fabsf(v[r]) : 0.f;
                    const int img = sImg[rl + (r & 3) + 8 * (r >> 2)];
                    if (img == img0) omax = fmaxf(omax, av);
                    else if (img == img0 + 1) omax1 = fmaxf(omax1, av);       // a tile that spans two images
                    else if (av > 0.f) cnl::report_max(a.ymax + img * AMS, av);  // maps smaller than the tile: rare rows
                }
            }
        }
    }
    if (a.ymax) {          // one vector atomic per wave for the tile's first image and one for the next
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            omax = fmaxf(omax, __shfl_xor(omax, o, 64));
            omax1 = fmaxf(omax1, __shfl_xor(omax1, o, 64));
        }
        if (lane == 0) cnl::report_max(a.ymax + img0 * AMS, omax);
        if (lane == 0 && img0 + 1 < a.N) cnl::report_max(a.ymax + (img0 + 1) * AMS, omax1);
    }
}

template <int WM, int WN, int TM, int TN>
static int launch_cfg(const PwArgs& in, hipStream_t stream) {
    using C = Cfg<WM, WN, TM, TN>;
    PwArgs a = in;
    a.tiles_n = (a.Cout + C::BN - 1) / C::BN;
    a.tiles = ((a.M + C::BM - 1) / C::BM) * a.tiles_n;
    static cnl::DeviceOnce once;            // one per instantiation
    const int rc = cnl::kernel_setup(once, reinterpret_cast<const void*>(&pointwise_kernel<WM, WN, TM, TN>), 160 * 1024);
    if (rc != CNL_OK) return rc;
    hipLaunchKernelGGL((pointwise_kernel<WM, WN, TM, TN>), dim3(a.tiles), dim3(C::THREADS), C::LDS_BYTES + C::BM * 16, stream, a);
    return cnl::check_launch("pointwise_kernel");
}

static void magic_u31(unsigned d, unsigned* magic, unsigned* shift) {
    if (d <= 1) { *magic = 0; *shift = 0xFFu; return; }
    unsigned s = 0;
    while ((1ull << s) < d) ++s;
    *magic = (unsigned)(((1ull << (31 + s)) / d) + 1);
    *shift = s - 1;
}

}  // namespace cnl_pw

// Tile shapes (algo = CNL_ALGO_FORCE + t pins one for A/B runs): 1 = 64 x 128, 2 = 128 x 128, 3 = 256 x 64.  Default: as conv_f16x2.hip —
// 256 x 64 for Cout <= 64, 64 x 128 while 128 x 128 tiles would not give 512 workgroups, else 128 x 128.  A function of the shape, never of N
// alone beyond the grid size; every tile shape sums the same products in the same chunk order, so the choice does not change any bit.
extern "C" int cnl_pointwise_nhwc_f32(const cnl_conv_params* p, const float* x2, int32_t H2, int32_t W2, int32_t C2, int32_t ldx2,
                                      int32_t stride2, const float* x2_absmax, void* stream) {
    using namespace cnl_pw;
    const char* who = "cnl_pointwise_nhwc_f32";
    CNL_REQUIRE(p, CNL_E_BAD_ARG, "%s: null params", who);
    CNL_REQUIRE(p->x && p->w && p->bias && p->y, CNL_E_BAD_ARG, "%s: null tensor pointer", who);
    CNL_REQUIRE(p->N > 0 && p->H_in > 0 && p->W_in > 0 && p->Cin > 0 && p->Cout > 0, CNL_E_BAD_ARG, "%s: non-positive dimension", who);
    CNL_REQUIRE(p->KH == 1 && p->KW == 1 && p->stride == 1 && p->pad == 0, CNL_E_UNSUPPORTED, "%s: 1x1 / stride 1 / pad 0 only (got %d x %d / %d / %d)",
                who, p->KH, p->KW, p->stride, p->pad);
    CNL_REQUIRE(p->algo == CNL_ALGO_AUTO || p->algo == CNL_ALGO_F2 || (p->algo > CNL_ALGO_FORCE && p->algo <= CNL_ALGO_FORCE + 3), CNL_E_UNSUPPORTED,
                "%s: algo %u (the kernel runs the fp16-split arithmetic only: AUTO / F2, or CNL_ALGO_FORCE + 1..3 to pin a tile shape)", who, p->algo);
    CNL_REQUIRE((p->flags & ~(uint32_t)(CNL_RELU | CNL_W_SPLIT)) == 0, CNL_E_UNSUPPORTED, "%s: flags 0x%x (CNL_RELU only)", who, p->flags);
    CNL_REQUIRE(p->flags & CNL_W_SPLIT, CNL_E_BAD_ARG, "%s: p->w must be a cnl_conv_split_weights_f32 buffer (flags |= CNL_W_SPLIT)", who);
    CNL_REQUIRE(p->x_absmax, CNL_E_BAD_ARG, "%s: x_absmax is required (per-image max |x1|)", who);
    CNL_REQUIRE(p->Cin % 32 == 0 && p->Cin <= 4096, CNL_E_UNSUPPORTED, "%s: Cin=%d (a multiple of 32, at most 4096)", who, p->Cin);
    CNL_REQUIRE(p->Cout <= 4096, CNL_E_UNSUPPORTED, "%s: Cout=%d > 4096", who, p->Cout);
    CNL_REQUIRE(p->ldx >= p->Cin && p->ldx % 4 == 0 && p->ldy >= p->Cout, CNL_E_BAD_ARG, "%s: pixel strides ldx=%d ldy=%d too small / misaligned",
                who, p->ldx, p->ldy);
    CNL_REQUIRE(!p->residual || p->ldr >= p->Cout, CNL_E_BAD_ARG, "%s: ldr=%d < Cout", who, p->ldr);
    CNL_REQUIRE(((uintptr_t)p->x & 15) == 0 && ((uintptr_t)p->w & 15) == 0, CNL_E_BAD_ARG, "%s: x and w must be 16-byte aligned", who);
    int K2 = 0;
    if (x2) {
        CNL_REQUIRE(x2_absmax, CNL_E_BAD_ARG, "%s: the second source needs x2_absmax", who);
        CNL_REQUIRE(stride2 == 1 || stride2 == 2, CNL_E_UNSUPPORTED, "%s: stride2=%d (1 or 2)", who, stride2);
        CNL_REQUIRE(C2 > 0 && C2 % 32 == 0 && p->Cin + C2 <= 4096, CNL_E_UNSUPPORTED, "%s: C2=%d (a multiple of 32, Cin + C2 <= 4096)", who, C2);
        CNL_REQUIRE(ldx2 >= C2 && ldx2 % 4 == 0 && ((uintptr_t)x2 & 15) == 0, CNL_E_BAD_ARG, "%s: ldx2=%d / x2 alignment", who, ldx2);
        CNL_REQUIRE(H2 > 0 && W2 > 0 && (H2 - 1) / stride2 + 1 == p->H_in && (W2 - 1) / stride2 + 1 == p->W_in, CNL_E_BAD_ARG,
                    "%s: x2 is %d x %d at stride %d, which does not give the %d x %d output", who, H2, W2, stride2, p->H_in, p->W_in);
        K2 = C2;
    }
    PwArgs a;
    a.x1 = p->x; a.x2 = x2; a.bias = p->bias; a.res = p->residual; a.y = p->y;
    a.xmax1 = p->x_absmax; a.xmax2 = x2 ? x2_absmax : nullptr; a.ymax = reinterpret_cast<unsigned*>(p->y_absmax);
    a.N = p->N; a.Ho = p->H_in; a.Wo = p->W_in; a.Cout = p->Cout;
    a.K = p->Cin + K2; a.KT1 = p->Cin / 32; a.KT = a.K / 32;
    a.ldx1 = p->ldx; a.ldx2 = x2 ? ldx2 : 0; a.ldy = p->ldy; a.ldr = p->ldr;
    a.H2 = x2 ? H2 : 0; a.W2 = x2 ? W2 : 0; a.s2 = x2 ? stride2 : 1;
    a.flags = p->flags;
    const size_t total = (size_t)a.Cout * a.K;
    a.wsplit = p->w + total;
    a.wscale = p->w + 2 * total;
    const long long M = (long long)a.N * a.Ho * a.Wo;
    CNL_REQUIRE(M < (1ll << 31) - 512, CNL_E_UNSUPPORTED, "%s: N*H*W too large", who);
    a.M = (int)M;
    const unsigned long long lim = 0xFFFFFF00ull;
    const unsigned long long x1b = ((unsigned long long)(M - 1) * a.ldx1 + p->Cin) * 4ull;
    const unsigned long long x2b = x2 ? (((unsigned long long)a.N * H2 * W2 - 1) * a.ldx2 + K2) * 4ull : 0ull;
    const unsigned long long yb = ((unsigned long long)(M - 1) * a.ldy + a.Cout) * 4ull;
    const unsigned long long rb = a.res ? ((unsigned long long)(M - 1) * a.ldr + a.Cout) * 4ull : 0ull;
    const unsigned long long wb = (unsigned long long)total * 4ull;
    CNL_REQUIRE(x1b < lim && x2b < lim && yb + 512ull * a.ldy * 4 < lim && rb + 512ull * a.ldr * 4 < lim && wb < lim, CNL_E_UNSUPPORTED,
                "%s: a tensor spans >= 4 GiB; split the batch", who);
    a.x1_bytes = (unsigned)x1b; a.x2_bytes = (unsigned)x2b; a.y_bytes = (unsigned)yb; a.r_bytes = (unsigned)rb; a.w_bytes = (unsigned)wb;
    magic_u31((unsigned)(a.Ho * a.Wo), &a.mg_hw, &a.sh_hw);
    magic_u31((unsigned)a.Wo, &a.mg_w, &a.sh_w);
    const hipStream_t s = (hipStream_t)stream;
    int t = p->algo > CNL_ALGO_FORCE ? (int)(p->algo - CNL_ALGO_FORCE) : 0;
    if (!t) {
        const long long tiles128 = ((M + 127) / 128) * ((a.Cout + 127) / 128);
        t = a.Cout <= 64 ? 3 : (tiles128 < 512 ? 1 : 2);
    }
    if (t == 3) return launch_cfg<4, 1, 2, 2>(a, s);      // 256 x 64
    if (t == 1) return launch_cfg<2, 2, 1, 2>(a, s);      //  64 x 128
    return launch_cfg<4, 1, 1, 4>(a, s);                  // 128 x 128
}
