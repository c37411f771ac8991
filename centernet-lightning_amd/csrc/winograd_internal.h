// The Winograd family's internal interface: every cnl_wino* function that one .hip defines and another calls is declared HERE and nowhere
// else, and every defining file includes this header (a drifted signature is a compile error, not a link-time surprise).  Behind the
// prototypes: the launch set-up that the row kernels (winograd9 / 10 / 13.hip, tools/experiments/winograd12.hip) share.
#pragma once
#include "cnl_common.h"

int cnl_wino2_launch(const cnl_conv_params* p, size_t u_floats, void* stream);     // winograd2.hip
size_t cnl_wino5_weight_bytes(int Cin, int Cout);                                  // winograd5.hip (winograd6.hip shares its weight layout, scales and scalars)
size_t cnl_wino5_scalar_floats();
int cnl_wino5_transform_weights(const float* w_ohwi, const float* u_f32, size_t u_f32_floats, void* u5, float* scal, int Cin, int Cout, void* stream);
int cnl_wino5_own_absmax(const cnl_conv_params* p, float* scal, void* stream);
int cnl_wino5_launch(const cnl_conv_params* p, const void* u5, float* scal, void* stream);
int cnl_wino6_launch(const cnl_conv_params* p, const void* u5, float* scal, void* stream);        // winograd6.hip
size_t cnl_wino9_weight_bytes(int Cin, int Cout);                                  // winograd9.hip
size_t cnl_wino9_scalar_floats(int Cin, int Cout);
int cnl_wino9_transform_weights(const float* w_ohwi, void* u9, float* isu, int Cin, int Cout, void* stream);
bool cnl_wino9_eligible(const cnl_conv_params* p);
size_t cnl_wino9_up_weight_bytes(int Cin, int Cout);                               // the row-pair weight sets of a conv behind a folded upsample (cnl_conv_params.w_up)
int cnl_wino9_up_transform_weights(const float* w_ohwi, void* u9, float* isu, int Cin, int Cout, void* stream);
int cnl_wino9_launch(const cnl_conv_params* p, const void* u9, const float* isu, const float* xmax, void* stream);
int cnl_wino_packed_stride(const cnl_conv_params* p);                               // packed rows of the F(2,3) row kernels
int cnl_wino_images_per_launch(const cnl_conv_params* p);                           // tensors of >= 4 GiB run in groups of images
void cnl_wino_sub_batch(const cnl_conv_params* p, int n0, int n, cnl_conv_params* q, const float** xmax);
bool cnl_wino10_eligible(const cnl_conv_params* p);                                // winograd10.hip (reads winograd9.hip's weights)
int cnl_wino10_launch(const cnl_conv_params* p, const void* u9, const float* isu, const float* xmax, bool cout32, void* stream);
size_t cnl_wino13_weight_bytes(int Cin, int Cout);                                 // winograd13.hip: F(4,3) along x (weights of its own: six transform positions)
size_t cnl_wino13_scalar_floats(int Cin, int Cout);
int cnl_wino13_transform_weights(const float* w_ohwi, void* u13, float* isu, int Cin, int Cout, void* stream);
bool cnl_wino13_eligible(const cnl_conv_params* p);
int cnl_wino13_launch(const cnl_conv_params* p, const void* u13, const float* isu, const float* xmax, void* stream);
#ifdef CNL_EXPERIMENTS      // tools/experiments/ (`make experiments`)
bool cnl_wino12_eligible(const cnl_conv_params* p);                                // winograd12.hip (round 5: Cin = 64, the epilogue rides in the next item's chunks)
int cnl_wino12_launch(const cnl_conv_params* p, const void* u9, const float* isu, const float* xmax, void* stream);
int cnl_wino1_launch(const cnl_conv_params* p, void* stream);                       // winograd1.hip
size_t cnl_wino3_weight_bytes(int Cin, int Cout);                                  // winograd3.hip
int cnl_wino3_transform_weights(const float* w_ohwi, void* u3, int Cin, int Cout, void* stream);
int cnl_wino3_launch(const cnl_conv_params* p, const void* u3, void* stream);
int cnl_wino4_launch(const cnl_conv_params* p, const void* u3, void* stream);        // winograd4.hip
int cnl_wino7_launch(const cnl_conv_params* p, const void* u5, float* scal, void* stream);        // winograd7.hip
#else
static inline size_t cnl_wino3_weight_bytes(int, int) { return 0; }
#endif

// ---- launch set-up of the row kernels ------------------------------------------------------------------------------------------------------
// The work-item shape of a row kernel: output rows, pixels of a block row and couts per item, and the slack its y / residual span check keeps
// behind the last pixel, in bytes per float of pixel stride (4: one pixel, the F(2,3) kernels' second store of a pair; 16: four, F(4,3)).
struct cnl_wino_row_tile { int rows, px, couts, slack; };

// floor(2^32 / d): item index -> coordinates by multiply-high + one correction (d = 1: the largest multiplier, the correction does the rest)
inline unsigned cnl_wino_magic(int d) { return d == 1 ? 0xFFFFFFFFu : (unsigned)(0x100000000ull / (unsigned)d); }

// Fills what the Args structs of the row kernels share (same field names; each kernel keeps its own struct and layout: winograd13 has no stored
// size / images per block row, winograd12 no chunk count, so there is no common base that would leave every layout as it is): tensors, sizes,
// the block grid with its magic divisors, the 32-bit spans, flags.  The caller sets its weight pointer and the fields only it has (Hs, Ws,
// ipb, lw, CC).  ipb: images side by side in a block row (1 where the kernel has no such form); pk: packed-row stride or 0; u_bytes: span of
// the weights.  Returns CNL_OK with a.blocks set, or CNL_E_UNSUPPORTED.
template <class A>
int cnl_wino_row_setup(A& a, const cnl_conv_params* p, const float* isu, const float* xmax, const cnl_wino_row_tile& t, int ipb, int pk, size_t u_bytes) {
    a.x = p->x; a.xmax = xmax; a.isu = isu; a.ymax = reinterpret_cast<unsigned*>(p->y_absmax);
    a.bias = p->bias; a.res = p->residual; a.y = p->y;
    const int upf = (p->flags & CNL_UPSAMPLE_IN) ? 2 : 1;
    a.Nimg = p->N; a.H = p->H_in * upf; a.W = p->W_in * upf; a.Cin = p->Cin; a.Cout = p->Cout;
    a.N = pk ? 1 : (p->N + ipb - 1) / ipb;
    a.pk = pk;
    a.m_pk = pk ? (unsigned)(0x100000000ull / (unsigned)pk) : 0u;
    a.CoutP = (p->Cout + 63) / 64 * 64;
    a.ldx = p->ldx; a.ldy = p->ldy; a.ldr = p->ldr;
    a.nb = a.CoutP / t.couts; a.bx = pk ? (int)(((long long)p->N * pk + t.px - 1) / t.px) : (a.W + t.px - 1) / t.px; a.by = (a.H + t.rows - 1) / t.rows;
    a.m_nb = cnl_wino_magic(a.nb); a.m_bx = cnl_wino_magic(a.bx); a.m_by = cnl_wino_magic(a.by);
    const long long blocks = (long long)a.N * a.by * a.bx * a.nb;
    CNL_REQUIRE(blocks < (1ll << 31), CNL_E_UNSUPPORTED, "cnl_conv3x3_winograd_f32: grid too large");
    a.blocks = (int)blocks;
    const unsigned long long xb = (((unsigned long long)p->N * p->H_in * p->W_in - 1) * p->ldx + p->Cin) * 4ull;
    const unsigned long long ub = (unsigned long long)u_bytes;
    const unsigned long long Mo = (unsigned long long)p->N * a.H * a.W;
    const unsigned long long yb = ((Mo - 1) * p->ldy + p->Cout) * 4ull;
    const unsigned long long rb = p->residual ? ((Mo - 1) * p->ldr + p->Cout) * 4ull : 0ull;
    const unsigned long long slack = (unsigned long long)t.slack;
    CNL_REQUIRE(xb < 0xFFFFFF00ull && ub < 0xFFFFFF00ull && yb + slack * p->ldy < 0xFFFFFF00ull && rb + slack * (p->residual ? p->ldr : 0) < 0xFFFFFF00ull,
                CNL_E_UNSUPPORTED, "cnl_conv3x3_winograd_f32: tensor spans >= 4 GiB; split the batch");
    a.x_bytes = (unsigned)xb; a.u_bytes = (unsigned)ub; a.y_bytes = (unsigned)yb; a.r_bytes = (unsigned)rb; a.b_bytes = (unsigned)p->Cout * 4u;
    a.flags = p->flags;
    return CNL_OK;
}

// A launch whose tensors span >= 4 GiB runs as groups of images (cnl_wino_images_per_launch), one call of `one(q, xmax of the group)` each.
template <class F>
int cnl_wino_image_groups(const cnl_conv_params* p, const float* xmax, F&& one) {
    const int per = cnl_wino_images_per_launch(p);
    CNL_REQUIRE(per > 0, CNL_E_UNSUPPORTED, "cnl_conv3x3_winograd_f32: one image of a tensor spans >= 4 GiB");
    for (int n0 = 0; n0 < p->N; n0 += per) {
        cnl_conv_params q;
        const float* xm = xmax;
        cnl_wino_sub_batch(p, n0, p->N - n0 < per ? p->N - n0 : per, &q, &xm);
        const int rc = one(&q, xm);
        if (rc != CNL_OK) return rc;
    }
    return CNL_OK;
}
