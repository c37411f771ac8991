/*
 * centernet_gfx950.h — C ABI of libcenternet_gfx950.so
 *
 * MI355X-native (gfx950 / CDNA4) replacement for the CenterNet inference hot path of
 * gau-nernst/centernet-lightning.  The reference is pure Python dispatching to ATen/cuDNN ops; every
 * entry point below replaces the ATen call sites listed beside it (paths relative to the reference
 * root).  The reference-side binding is a ctypes stub.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers (HBM); all tensors are fp32 unless stated;
 *   - activations are NHWC ("channels_last"): element (n,y,x,c) lives at ((n*H+y)*W+x)*ld + c where
 *     ld >= C is the pixel stride in elements (lets several heads share one buffer);
 *   - conv weights are OHWI: w[co][ky][kx][ci], K = KH*KW*Cin contiguous per output channel, with the
 *     eval-mode BatchNorm already folded in (scale into w, shift into bias);
 *   - every call is asynchronous on the hipStream_t passed as `stream` (void* to keep HIP headers out
 *     of the binding), allocates nothing, and is re-entrant;
 *   - return value: 0 = CNL_OK, negative = CNL_E_*; cnl_last_error() returns the message of the last
 *     failure on the calling thread.  No C++ exception crosses this boundary.
 */
#ifndef CENTERNET_GFX950_H
#define CENTERNET_GFX950_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the entry points declared in this header are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CNL_ABI_VERSION 13   /* 13: CNL_ALGO_F43 + kernel variant 13 (csrc/winograd13.hip: 1-D Winograd F(4,3) along x on the fp16-split arithmetic; its weight pieces are a new tail of the transformed-weight buffer, so cnl_winograd_weight_floats grows for Cin % 32 == 0); 12: cnl_conv_params.w_up + cnl_winograd_up_weight_floats / cnl_winograd_transform_weights_up_f32 (a 3x3 conv behind a folded nearest-2x upsample: pre-summed row-pair weights, two instead of three kernel rows per output row), cnl_sizeof_params (a binder's struct-layout check); 11: cnl_conv_params.fuse_w / fuse_part + cnl_fused_out_pack_weights_f32 / cnl_fused_out_reduce_f32 (a 1x1 conv of <= 4 channels folded into the 3x3 launch before it); the row-Winograd kernels take maps of any even width in packed rows and tensors of >= 4 GiB in groups of images; CNL_ALGO_FORCE + 32 + v; 10: per-image maxima arrays are strided (cnl_absmax_stride() = 32 floats: one cache line per image); the stem entry points take y_absmax; CNL_ALGO_LATENCY and the half-height row-Winograd kernel (csrc/winograd10.hip, variants 10 / 11); the F(4x4,3x3) split kernel is gone (CNL_ALGO_F4, CNL_WINO_F16X2_F4, cnl_winograd_f4_weight_floats, cnl_winograd_transform_weights_f4_f32 removed: slower than the row-Winograd default at 4x its rounding error); 9: CNL_W_SPLIT + cnl_conv_split_weight_floats / cnl_conv_split_weights_f32 (pre-split weights for the fp16-split direct convs); 8: cnl_track_frame_f32 / cnl_track_frame_bytes (one self-describing record per frame, writable straight into mapped host memory), cnl_host_alloc / cnl_host_free; 7: the F(4x4) weight copy is an optional tail of the transformed-weight buffer (cnl_winograd_f4_weight_floats, cnl_winograd_transform_weights_f4_f32), cnl_conv3x3_winograd_variant, row-Winograd kernel behind CNL_WINO_F16X2; 6: cnl_conv_params.splitk / splitk_scratch (reduction split for small grids), cnl_fuse_sum_nhwc_f32; 5: cnl_conv_params.algo (arithmetic class per launch instead of process-wide environment switches), Winograd F(4x4,3x3) kernel, cnl_stem_conv7x7_f32 takes algo, uint8 stem + resize entry points; 4: cnl_conv_params.w_absmax, cnl_conv2d_kernel, cnl_absmax_per_image_f32 (fp16-split direct conv); 3: cnl_conv_params carries x_absmax / y_absmax (tensor-maximum hand-over between conv launches); 2: stem packed weights are [154][64] (cnl_stem_packed_weight_floats), neck-option / tracker / format entry points */

enum {
    CNL_OK = 0,
    CNL_E_BAD_ARG = -1,      /* null pointer, non-positive dimension, inconsistent shapes            */
    CNL_E_UNSUPPORTED = -2,  /* shape outside what the gfx950 kernels cover (e.g. Cin % 32 != 0)     */
    CNL_E_WORKSPACE = -3,    /* workspace pointer null / too small (see cnl_decode_workspace_bytes)  */
    CNL_E_HIP = -4           /* a HIP runtime call failed; text in cnl_last_error()                  */
};

/*
 * cnl_conv_params.algo / the `algo` argument of cnl_stem_conv7x7_f32: the ARITHMETIC CLASS the caller allows for a launch.  Inside a class
 * the kernel is a function of the layer shape and the hints alone — never of the batch size, never of the environment.
 *   CNL_ALGO_AUTO  the default.  fp32 in / fp32 accumulate / fp32 out everywhere; where it pays, each fp32 product is formed on the fp16
 *                  matrix cores from a scaled two-way fp16 split of both operands (three cross terms): every kernel's error against
 *                  float64 is at or below the fp32 matrix core's (tests/test_gpu_conv.py pins that per kernel).
 *   CNL_ALGO_F2    synonym of CNL_ALGO_AUTO (Winograd tiles no larger than F(2x2,3x3)).
 *   CNL_ALGO_F32   fp32 matrix cores only (v_mfma_f32_32x32x2_f32), no split operands anywhere; hints are ignored.
 *   CNL_ALGO_LATENCY  cnl_conv3x3_winograd_f32 only: AUTO's arithmetic on small work items (csrc/winograd10.hip: 4 rows x 64 pixels x 32 couts, two
 *                  workgroups per CU) wherever the row-Winograd kernels apply — for one-image batches, where the default's 8-row x 64-cout items leave
 *                  most CUs idle (a 256 -> 256 conv on a 32 x 32 map: 46 -> 23 us).  Same bits as AUTO wherever AUTO takes a row-Winograd kernel.
 *   CNL_ALGO_F43   cnl_conv3x3_winograd_f32 only (ABI v13): AUTO's choices, except that a 3x3 / stride-1 layer with Cin >= 128 on a map at least 128 pixels wide that the 4-row x 128-pixel
 *                  items of csrc/winograd13.hip tile well (padding <= 1.35 x; packed rows included) runs as 1-D Winograd F(4,3) along x — 108 instead of
 *                  144 matrix instructions per 16-channel chunk, the same split arithmetic, interpolation points {0, -1, 1, 1/2, -2, inf}.  The larger tile's
 *                  transforms amplify rounding: error against float64 2.4-4.6 x the fp32 matrix core's (tests/test_gpu_conv.py pins <= 6 x), inside the
 *                  path's 1e-4 by two orders of magnitude but above AUTO's promise — hence a class of its own, never what AUTO takes.  Batch-invariant.
 *   CNL_ALGO_FORCE + v  tests / A-B measurements: pin kernel variant v (2, 5, 6, 9, 10, 11, 13; 1, 3, 4, 7 in `make experiments` builds) wherever
 *                  it can run at all.  A launch v cannot take — a shape, stride or alignment outside its eligibility rule — is NOT an error: it runs
 *                  the nearest variant that can (9 / 10 / 11 -> 5; 13 -> 9, else 5; 6 with Cout % 128 != 0 -> 5; Cin % 16 != 0 -> 2), correctly,
 *                  and cnl_conv3x3_winograd_variant reports which.  The one exception is a launch with fuse_w, which only variant 9 implements:
 *                  it fails with CNL_E_UNSUPPORTED and writes nothing (tests/test_gpu_strided_io.py pins both).
 */
enum {
    CNL_ALGO_AUTO = 0,
    CNL_ALGO_F2 = 1,
    CNL_ALGO_F32 = 2,                /* (3 was CNL_ALGO_F4 until ABI v9: rejected now) */
    CNL_ALGO_LATENCY = 4,
    CNL_ALGO_F43 = 5,
    CNL_ALGO_FORCE = 100
};

/* epilogue / gather flags of cnl_conv2d_nhwc_f32 */
enum {
    CNL_RELU = 1u << 0,          /* y = max(y, 0)                      nn.ReLU      (layers.py:75)        */
    CNL_SIGMOID = 1u << 1,       /* y = 1/(1+exp(-y))                  .sigmoid()   (centernet.py:205)    */
    CNL_UPSAMPLE_IN = 1u << 2,   /* read x through nn.Upsample(scale_factor=2, mode="nearest")
                                    (layers.py:99): logical input is (2*H_in, 2*W_in)                   */
    CNL_UPSAMPLE_OUT_ADD = 1u << 3, /* write y at 2x resolution and add `residual` there:
                                    y[n,2oy+dy,2ox+dx,:] = conv(x)[n,oy,ox,:] + bias + residual[...]
                                    = Fuse.forward's project -> resize("up") -> sum (layers.py:160-174) */
    CNL_RELU6 = 1u << 4,         /* y = min(max(y, 0), 6)              nn.ReLU6     (layers.py:62,66; separable conv);
                                    cnl_conv2d_nhwc_f32 / cnl_deconv2x_nhwc_f32 / cnl_depthwise3x3_nhwc_f32 only      */
    CNL_W_SPLIT = 1u << 5        /* cnl_conv2d_nhwc_f32: p->w is a cnl_conv_split_weights_f32 buffer (the fp32 OHWI weights followed by
                                    their scaled fp16 split): the fp16-split direct kernel reads the pieces instead of splitting
                                    the weights of every chunk again — same bits out; kernels that do not split ignore the tail   */
};

/*
 * One fused convolution layer: Conv2d (+ folded BatchNorm2d) (+ residual add) (+ ReLU | sigmoid).
 * Replaces, per call site:
 *   - ResNet BasicBlock conv3x3/BN/ReLU and the 1x1 stride-2 downsample (torchvision, reached through
 *     backbone.forward_features, models/meta.py:42);
 *   - make_conv(..., conv_type="normal")            models/layers.py:72-77
 *   - Fuse.project 1x1 conv with bias               models/layers.py:152
 *   - GenericHead block_i (ConvBnAct) and out_conv  models/meta.py:24-30
 * Implementation: fp32 MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM, M = N*Ho*Wo, N = Cout,
 * K = KH*KW*Cin, LDS-staged via buffer_load ... lds.
 */
typedef struct cnl_conv_params {
    const float* x;         /* input  [N, H_in, W_in, ldx]                                           */
    const float* w;         /* weight [Cout, KH, KW, Cin]                                            */
    const float* bias;      /* [Cout] (never null; zeros when the layer has none)                    */
    const float* residual;  /* null, or same geometry as y with pixel stride ldr                      */
    float* y;               /* output [N, H_out, W_out, ldy]                                         */
    int32_t N, H_in, W_in, Cin, Cout;
    int32_t KH, KW, stride, pad;
    int32_t ldx, ldy, ldr;  /* pixel strides in elements                                             */
    /* Layout rules of the conv entry points (cnl_conv2d_nhwc_f32, cnl_conv3x3_winograd_f32, cnl_conv3x3_up2_nhwc_f32, cnl_pointwise_nhwc_f32,
     * cnl_deconv2x_nhwc_f32; pinned by tests/test_gpu_strided_io.py).  INPUT: ldx >= Cin, ldx % 4 == 0 and x 16-byte aligned (likewise ldx2 / x2),
     * else CNL_E_BAD_ARG (cnl_conv3x3_winograd_f32: CNL_E_UNSUPPORTED for the stride) before anything is launched.  OUTPUT and RESIDUAL: any
     * ldy >= Cout, ldr >= Cout and any 4-byte aligned y / residual are accepted, so a tensor may be a channel slice at any offset of a wider
     * buffer.  A launch writes the Cout channels of its N * H_out * W_out pixels and NOTHING else: not the other ldy - Cout channels of a pixel,
     * not a byte behind the last pixel.  The result does not depend on the layout as long as the same kernel runs; the kernels with 16-byte
     * epilogues are chosen only where Cout % 4 == 0, ldy % 4 == 0, y is 16-byte aligned and, with a residual, ldr % 4 == 0 and the residual is
     * 16-byte aligned (the row-Winograd variants 9 / 10 / 11 / 13 — another layout runs variant 2 / 5 / 6, other arithmetic of the same class
     * promise — and the vector epilogue of CNL_UPSAMPLE_OUT_ADD, whose scalar form gives the same bits).  The elementwise entry points
     * (cnl_upsample2x / cnl_fuse_sum / cnl_depthwise3x3) ask for every stride % 4 == 0 and every pointer 16-byte aligned and refuse anything else. */
    uint32_t flags;         /* CNL_RELU | CNL_SIGMOID | CNL_UPSAMPLE_IN | CNL_UPSAMPLE_OUT_ADD        */
    /* Optional hand-over of the per-image maximum magnitude of a tensor between launches (cnl_conv3x3_winograd_f32 only; NULL =
     * unused).  Both point to N * cnl_absmax_stride() floats: image n's value sits at element n * cnl_absmax_stride() (32 floats = one 128-byte line
     * per image since ABI v10, see cnl_absmax_stride() below; an array of N packed floats is OUT OF BOUNDS for n > 0).  The fp16-split Winograd kernel scales each image's input by a power of two
     * derived from max |x| of THAT image (an image's result never depends on its batch neighbours): with x_absmax it reads the
     * maxima from device memory instead of making its own pass over x.  A producer given y_absmax folds max |y| of everything it
     * stores for image n into y_absmax[n * cnl_absmax_stride()] (atomic max on the bit pattern: zero the array on the stream before the producer
     * runs); the fp16-split kernels honour it, and so does cnl_conv2d_nhwc_f32's CNL_UPSAMPLE_OUT_ADD epilogue (fp32 matrix cores; FPN Fuse: the 3x3 output
     * conv behind it consumes the figure); the other fp32-matrix-core launches ignore it.  A maximum over a superset of the consumer's
     * channels is a valid, slightly conservative bound.  GUARANTEED RANGE of the split arithmetic: one scale per image means a value 2^-n below
     * the image's maximum keeps min(22, 38 - n) significant bits — outputs whose inputs lie within 1e4 of the image maximum are at the fp32
     * matrix core's error level, at 1e6 the error is 2-6e-5 of the LOCAL output magnitude (inside the path's 1e-4), beyond that pass
     * CNL_ALGO_F32 (tests/test_gpu_conv.py::test_split_arithmetic_with_an_outlier_inside_one_image).  WITHOUT x_absmax a launch of the fp16-split kernels takes at most 1024 images (4096 up
     * to ABI v9: the private scratch of the own pass is strided like every maxima array now); more return CNL_E_UNSUPPORTED.
     * NON-FINITE VALUES (every entry point of this header that takes a batch of activations — the convs, the stems, the pointwise kernel, the
     * deconv, the elementwise and sampling launches, the folded out_conv and its reduce): NaN or Inf in image n — in x, the residual, a second
     * source, or in image n's x_absmax line — leave image n's OWN outputs and its max |y| line unspecified.  They may even come out finite and
     * plausible: ReLU is an IEEE maximum (fmaxf(NaN, 0) = 0), and a maximum of 0, Inf or NaN takes scale 1.  They NEVER change a bit of another
     * image's outputs, of its max |y| line, or of its rows of splitk_scratch / fuse_part, whatever tile, block row or work item the images
     * share (tests/test_gpu_nonfinite.py: NaN, +-Inf and overflowing values in one image ahead of every launch of every plan form).  Nothing
     * here reports them: engine.KernelOptions(check_range=True) is the way to find them (it refuses NaN / Inf in the fp32 network input and in
     * every fp16-split launch's input with the launch and the image named).
     *                                                                        */
    const float* x_absmax;
    float* y_absmax;
    /* cnl_conv2d_nhwc_f32 only: device pointer to ONE float, max |w| of this layer's weights (e.g. computed once when the weights
     * are loaded), or NULL.  With both x_absmax and w_absmax the 1x1 / 3x3 convs without up-sampling flags form each fp32 product
     * on the fp16 matrix cores from scaled two-way splits of both operands (csrc/conv_f16x2.hip: same error against float64 as
     * the fp32 matrix-core kernel, 2-3x faster) and honour y_absmax; without them the fp32 matrix-core kernel runs.             */
    const float* w_absmax;
    uint32_t algo;          /* CNL_ALGO_* (0 = CNL_ALGO_AUTO)                                                                       */
    /* cnl_conv2d_nhwc_f32 only, optional (0 / NULL = off): split the reduction (KH*KW*Cin) over `splitk` workgroups per output tile —
     * for launches whose output is too small to fill the chip (one image, 16x16 .. 32x32 maps): slice s writes its partial sums to
     * splitk_scratch[s][N*Ho*Wo][Cout] (cnl_conv2d_splitk_scratch_bytes()), a second kernel adds the slices IN SLICE ORDER (deterministic)
     * and applies bias / residual / activation / y_absmax.  Honoured where the fp16-split kernel runs (x_absmax and w_absmax given,
     * 1x1 or 3x3, no CNL_UPSAMPLE_*); elsewhere the launch runs unsplit.  The result depends on `splitk` (summation grouping), so a
     * caller that needs shard == full batch bit for bit must choose it from the layer shape alone.                                  */
    int32_t splitk;
    float* splitk_scratch;
    size_t splitk_scratch_bytes;
    /* cnl_conv3x3_winograd_f32 only, optional (NULL = off; ABI v11): a following 1x1 convolution with at most 4 output channels — the box-size
     * head's out_conv behind its last 3x3 block (reference models/meta.py:24-30) — folded into THIS launch: besides y, the epilogue writes
     * fuse_part[b][pixel][0..3] = sum over the 32 channels co of block b (co in [32 b, 32 b + 32)) of y[pixel][co] * fuse_w[co][0..3]
     * (fp32, fixed order), for b < ceil(Cout / 64) * 2; cnl_fused_out_reduce_f32 then adds the blocks in order, adds the bias and applies the
     * activation: the 1x1 conv never re-reads the 3x3 conv's output (C1: a 537 MB read, 110 us).  fuse_w: [ceil(Cout / 64) * 64][4] floats,
     * rows >= Cout and columns >= the 1x1 conv's channel count zero (cnl_fused_out_pack_weights_f32); fuse_part: ceil(Cout / 64) * 2 *
     * N * H * W * 4 floats.  Implemented by ONE kernel: the row-Winograd variant 9 (csrc/winograd9.hip).  The dispatcher keeps a launch that
     * carries fuse_w on variant 9 wherever its AUTO / LATENCY / F43 choice would have been another ROW kernel (10 / 11 / 13), but a shape it routes elsewhere
     * (e.g. N = 32, 16 x 16, 512 -> 512: variant 5) fails with CNL_E_UNSUPPORTED — a caller must check cnl_conv3x3_winograd_variant(p) == 9 WITH fuse_w set
     * before relying on the fold (engine.py does).  Deterministic, batch-invariant. */
    const float* fuse_w;
    float* fuse_part;
    /* cnl_conv3x3_winograd_f32 with CNL_UPSAMPLE_IN only, optional (NULL = off; ABI v12): the ROW-PAIR weights of this layer
     * (cnl_winograd_transform_weights_up_f32).  Behind a nearest-2x upsample (make_upsample + ConvBnAct: reference models/layers.py:99,72-77 — the first
     * block of every head behind the simple neck, models/meta.py:24-26) the image rows 2j and 2j+1 are the same source row, so the three kernel rows of an
     * output row meet two distinct input rows: out[2m] = row[2m-1] g0 + row[2m] (g1 + g2), out[2m+1] = row[2m] (g0 + g1) + row[2m+2] g2.  With the four
     * pre-summed sets the row-Winograd kernel (variant 9) issues 96 instead of 144 matrix instructions per 16-channel chunk.  Results: within fp32
     * rounding of the launch without w_up (another grouping of the same products), deterministic, batch-invariant — a function of the shape and of w_up
     * being given.  Ignored (the general form runs) with a residual, with fuse_w, and by every other kernel.                                        */
    const float* w_up;
} cnl_conv_params;

/* The 1x1 conv folded into a 3x3 launch (cnl_conv_params.fuse_w / fuse_part): w_ohwi [C2][Cout] (C2 <= 4) -> fuse_w [ceil(Cout/64)*64][4];
 * and its second half: y[pixel][c] = act(bias[c] + sum_b part[b][pixel][c]), b in order, for M pixels (pixel stride ldy floats, c < C2;
 * flags: CNL_SIGMOID | CNL_RELU).                                                                                                       */
int cnl_fused_out_pack_weights_f32(const float* w_ohwi, float* fuse_w, int32_t Cout, int32_t C2, void* stream);
int cnl_fused_out_reduce_f32(const float* part, int32_t nblocks, int64_t M, int32_t C2, const float* bias, float* y, int32_t ldy,
                             uint32_t flags, void* stream);
int cnl_conv2d_nhwc_f32(const cnl_conv_params* p, void* stream);
/* The row-pair weights of cnl_conv_params.w_up: w_ohwi [Cout][3][3][Cin] (BatchNorm folded) -> u_up, cnl_winograd_up_weight_floats(Cin, Cout) floats
 * (0: Cin % 32 != 0, no such form): [Cin/16][4 positions][4 sets g0, g0+g1, g1+g2, g2][2 fp16 pieces][ceil(Cout/64)*64][16] + one inverse scale per cout. */
size_t cnl_winograd_up_weight_floats(int32_t Cin, int32_t Cout);
int cnl_winograd_transform_weights_up_f32(const float* w_ohwi, float* u_up, int32_t Cin, int32_t Cout, void* stream);
size_t cnl_conv2d_splitk_scratch_bytes(const cnl_conv_params* p);   /* for p->splitk slices; 0 when splitk <= 1 */

/* Which kernel cnl_conv2d_nhwc_f32 takes for *p (a function of the hints, kernel size and flags only — never of the batch). */
#define CNL_CONV_F32 2     /* fp32 matrix cores (csrc/conv_mfma.hip); ignores y_absmax                                    */
#define CNL_CONV_F16X2 5   /* fp16 matrix cores, scaled two-way split (csrc/conv_f16x2.hip); writes y_absmax when given   */
int cnl_conv2d_kernel(const cnl_conv_params* p);

/*
 * 3x3 / stride 1 / pad 1 conv on the nearest-2x upsampled input (nn.Upsample(scale_factor=2) + ConvBnAct: models/layers.py:99,72-77;
 * the first head block behind the simple neck, models/meta.py:24-26) computed as four 2x2 sub-pixel phase convolutions on the
 * LOW-resolution input (16 instead of 36 multiplies per 2x2 output block; see csrc/conv_mfma.hip).  Same cnl_conv_params as
 * cnl_conv2d_nhwc_f32 with flags = CNL_UPSAMPLE_IN (| CNL_RELU | CNL_RELU6), KH = KW = 3, stride 1, pad 1, no residual; H_in / W_in
 * are the LOW-resolution size, y is [N, 2 H_in, 2 W_in, Cout].  p->w: the buffer cnl_up2_pack_weights_f32 fills from the OHWI
 * [Cout][3][3][Cin] weights (Cin % 32 == 0; cnl_up2_weight_floats sizes it): the phase weights [4][Cout][2][2][Cin] in fp32, the
 * same as scaled two-way fp16 split in the kernel's LDS row layout, and the scale.  With x_absmax the phases run on the fp16-split
 * kernel with the pre-split weights (cnl_conv3x3_up2_kernel reports CNL_CONV_F16X2; w_absmax is not needed) and y_absmax is
 * honoured; otherwise on the fp32 matrix cores.
 */
/*
 * Weights of a direct conv (square 1x1 / 3x3 kernel, Cin % 32 == 0) with their fp16 split appended, for flags |= CNL_W_SPLIT:
 * w_buf = [Cout*KH*KW*Cin fp32 OHWI weights (copied from w_ohwi unless w_buf == w_ohwi)][the same count of (hi, lo) fp16 pairs, scaled by the
 * power of two S_w = 2^(14 - e) of max |w| = m 2^e, in the B-row layout of the kernel][S_w + 3 pad floats];
 * cnl_conv_split_weight_floats sizes it (0: shape not supported).  Replaces nothing in the reference: it is the weight half of the
 * operand split that round 2's kernel redid for every 32-channel chunk of every launch (half of its VALU work on the stride-2 3x3 convs).
 */
size_t cnl_conv_split_weight_floats(int32_t Cin, int32_t Cout, int32_t KH, int32_t KW);
int cnl_conv_split_weights_f32(const float* w_ohwi, float* w_buf, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, void* stream);
/*
 * 1x1 convolution over NHWC rows as one GEMM [N*H*W, K] x [K, Cout] (torchvision Bottleneck.conv1 / conv3 / downsample of ResNet-50 / 101)
 * on the fp16-split arithmetic (csrc/pointwise.hip), with a TWO-SOURCE form for a stage's conv3 and its downsample in one launch:
 *     y = act(x1 W1 + x2[:, ::stride2, ::stride2, :] W2 + bias (+ residual))
 * p: KH = KW = 1, stride 1, pad 0; x = x1 [N, H_in, W_in, ldx] with Cin channels; y [N, H_in, W_in, ldy]; flags = CNL_W_SPLIT (| CNL_RELU);
 * p->w is a cnl_conv_split_weights_f32 buffer of the [Cout][Cin + C2] weights ([W1 | W2] concatenated along K, KH = KW = 1), p->bias holds
 * the summed biases; x_absmax (required) / y_absmax as in cnl_conv_params; residual / ldr optional; algo AUTO / F2, or CNL_ALGO_FORCE + t to
 * pin tile shape t (1: 64 x 128, 2: 128 x 128, 3: 256 x 64; same bits); CNL_ALGO_F32 is CNL_E_UNSUPPORTED.  x2 = NULL: single source (H2, W2,
 * C2, ldx2, stride2, x2_absmax ignored).  Otherwise x2 [N, H2, W2, ldx2] with C2 channels, (H2 - 1) / stride2 + 1 == H_in (likewise W),
 * stride2 1 or 2, x2_absmax its per-image maxima.  Both sources share ONE power-of-two scale per image, from the larger of the two maxima
 * (error bound: DESIGN.md §11).  Cin, C2: multiples of 32, Cin + C2 <= 4096; Cout <= 4096; any N*H*W.  Batch-invariant, deterministic.
 */
int cnl_pointwise_nhwc_f32(const cnl_conv_params* p, const float* x2, int32_t H2, int32_t W2, int32_t C2, int32_t ldx2, int32_t stride2,
                           const float* x2_absmax, void* stream);
size_t cnl_up2_weight_floats(int32_t Cin, int32_t Cout);
int cnl_up2_pack_weights_f32(const float* w_ohwi, float* w_packed, int32_t Cin, int32_t Cout, void* stream);
int cnl_conv3x3_up2_nhwc_f32(const cnl_conv_params* p, void* stream);
int cnl_conv3x3_up2_kernel(const cnl_conv_params* p);

/* The per-image maxima arrays of this API (cnl_conv_params.x_absmax / y_absmax, the stems' y_absmax, `out` below) hold image n's value at
 * element n * cnl_absmax_stride() — 32 floats apart since ABI v10: ONE 128-byte line per image.  (Every wave of a launch folds its maximum
 * into these with device-scope atomics, which the memory side resolves line by line: packed into one line, as in ABI <= 9, the reports of all
 * images queue behind each other.)  An array therefore has N * cnl_absmax_stride() floats; the elements between the slots are never read. */
int cnl_absmax_stride(void);
/* out[n * cnl_absmax_stride()] = max |x[n, :, 0:C]| over the `pixels` pixels of image n (pixel stride ld floats; C % 4 == 0, ld % 4 == 0, x
 * 16-byte aligned): the x_absmax hint for callers whose producer does not report it.  Zeroes the array first (stream-ordered).           */
int cnl_absmax_per_image_f32(const float* x, int32_t N, int64_t pixels, int32_t C, int32_t ld, float* out, void* stream);

/* Output spatial size of the conv itself (before CNL_UPSAMPLE_OUT_ADD doubles it). */
int cnl_conv2d_out_hw(const cnl_conv_params* p, int32_t* H_out, int32_t* W_out);

/*
 * The same fused layer for 3x3 / stride 1 / pad 1 (ResNet BasicBlock convs, make_conv, GenericHead blocks) computed by
 * Winograd F(2x2,3x3): 2.25x fewer matrix-core multiplies, same result up to fp32 rounding (see csrc/winograd.hip).
 * `p->w` must point to the PRE-TRANSFORMED weights produced by cnl_winograd_transform_weights_f32 from the OHWI
 * (BN-folded) weights; flags: CNL_RELU only (upsample / sigmoid variants stay on cnl_conv2d_nhwc_f32). Cin % 8 == 0.
 *
 * Several multiplier arrays serve this entry point, chosen from the layer SHAPE and p->algo (never the batch size): the fp32 matrix
 * core (csrc/winograd2.hip), or — where the channel loop is long (Cin >= 128 or Cout >= 256, Cin % 16 == 0) — the fp16 matrix core
 * fed with a two-way fp16 split of both fp32 operands under a per-image power-of-two scale (three cross terms, fp32
 * accumulation: csrc/winograd5.hip, winograd6.hip; measured error at or below the fp32 matrix core's, half-precision rate = 16x), as
 * F(2x2,3x3).  Round 3: wherever
 * 8-row x 64-pixel work items pad the map by less than 1.5x (Cin % 32 == 0, Cout % 4 == 0), the same split arithmetic runs as 1-D Winograd
 * F(2,3) along x with the three kernel rows in the reduction (csrc/winograd9.hip: per-output-channel weight scales; 0.5-0.8x the time of the
 * 2-D kernels, rounding error below theirs) — same class CNL_WINO_F16X2.
 * cnl_conv3x3_winograd_kernel reports which class a layer takes.  The fp16-split kernels without the x_absmax hint make their own
 * pass over the input and park the per-image maxima in the layer's weight buffer: such hint-less launches of ONE layer must not
 * run concurrently on two streams (launches that carry x_absmax — everything engine.py issues — have no hidden state).
 */
#define CNL_WINO_F32 2
#define CNL_WINO_BF16X3 3      /* experiment builds only */
#define CNL_WINO_F16X2 5
int cnl_conv3x3_winograd_f32(const cnl_conv_params* p, void* stream);
int cnl_conv3x3_winograd_kernel(const cnl_conv_params* p);            /* CNL_WINO_* for this layer shape, < 0: error code */
int cnl_conv3x3_winograd_variant(const cnl_conv_params* p);           /* the kernel behind the class (reporting only): 2 winograd2, 5 / 6 winograd5 / 6
                                                                         [F(2x2,3x3)], 9 winograd9 [F(2,3) along x, kernel rows
                                                                         in the reduction: 2/3 of the direct conv's multiplies], 10 / 11 winograd10
                                                                         [the same on 4-row x 64- / 32-cout items: bit for bit winograd9's
                                                                         output — the class never depends on N, but a launch of at most
                                                                         128 winograd9 items takes 11], 13 winograd13 [F(4,3) along x: 1/2 of the
                                                                         direct conv's multiplies; CNL_ALGO_F43 / FORCE + 13 only]; < 0: error code */
size_t cnl_winograd_weight_floats(int32_t Cin, int32_t Cout);        /* elements of the transformed weight buffer */
int cnl_winograd_transform_weights_f32(const float* w_ohwi, float* u, int32_t Cin, int32_t Cout, void* stream);
/*
 * Step before the path: uint8 HWC frames -> normalised fp32 NHWC, replacing albumentations
 * A.Normalize + ToTensorV2 of the reference's inference pre-processing (README.md:79-87, datasets/utils.py:9-21):
 * y = (float(x) - mean255[c]) * inv_std255[c], with HOST arrays mean255 = mean*255, inv_std255 = 1/(std*255) (3 floats each).
 * x: [N,H,W,3] u8, 4-byte aligned; y: [N,H,W,3] f32, 16-byte aligned (CNL_E_BAD_ARG otherwise; feed cnl_stem_conv7x7_f32 with strides
 * sn=H*W*3, sc=1, sh=W*3, sw=3).
 */
int cnl_normalize_u8_nhwc_f32(const uint8_t* x, float* y, int32_t N, int32_t H, int32_t W, const float* mean255,
                              const float* inv_std255, void* stream);

/*
 * albumentations A.Resize(height, width) = cv2.resize(img, (W_out, H_out), interpolation=cv2.INTER_LINEAR) on uint8 HWC frames
 * (README.md:84; datasets/utils.py:24-33 build the same pipeline for training): OpenCV's 8-bit fixed-point bilinear rule (half-pixel
 * centres, 11-bit coefficients, the two-stage rounding of VResizeLinear<uchar>), restated in csrc/preprocess.hip.
 * x: [N, H_in, W_in, C] u8 -> y: [N, H_out, W_out, C] u8, C <= 4.  Any byte alignment.
 */
int cnl_resize_bilinear_u8(const uint8_t* x, uint8_t* y, int32_t N, int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out,
                           int32_t C, void* stream);

/*
 * Batch entry for frames of DIFFERENT sizes: keep-aspect resize + centred constant border, the reference's validation transforms
 * (configs/centernet.yaml val_data.transforms; albumentations LongestMaxSize for a square target, then
 * PadIfNeeded(position="center") with a CONSTANT border) for N frames in ONE launch, and the way back for the decoded boxes
 * (datasets/inference.py carries original_height / original_width for that).
 *
 * `table` is a device array of N records, one per frame, 40 bytes each, 8-byte aligned:
 *     offset  0  const void* src    the frame's first pixel (uint8, HWC, C channels; device memory)
 *     offset  8  int32 h, w         frame size, >= 1
 *     offset 16  int32 row_stride   bytes from one source row to the next (>= w * C)
 *     offset 20  int32 new_h, new_w size of the resized frame inside the canvas, 1..height / 1..width
 *     offset 28  int32 pad_top, pad_left   where the resized frame starts: pad_top + new_h <= height, pad_left + new_w <= width
 *     offset 36  int32 reserved     0
 * Geometry rule of the Python host (letterbox_geometry): r = min(height / h, width / w) in double, new_h = min(height,
 * max(1, round_half_even(h * r))), new_w alike, pad_top = (height - new_h) / 2, pad_left = (width - new_w) / 2 (the remainder goes
 * to the bottom / right).  The kernel takes whatever window the record names.
 *
 * out: [N, height, width, C] u8, height and width positive multiples of 32, C in 1..4, 4-byte aligned.  Inside a frame's window the
 * bytes are those of the 8-bit resize entry point above for that frame resized to (new_h, new_w); outside it, byte c of every pixel
 * is bits 8c..8c+7 of fill_rgba.  Every byte of `out` is written exactly once (no memset needed before it); a frame's result depends
 * on that frame's record only.  N = 0 is a no-op.
 */
typedef struct cnl_letterbox_frame {
    const void* src;
    int32_t h, w;
    int32_t row_stride;
    int32_t new_h, new_w;
    int32_t pad_top, pad_left;
    int32_t reserved;
} cnl_letterbox_frame;
int cnl_letterbox_bilinear_u8(const void* table, uint8_t* out, int32_t N, int32_t height, int32_t width, int32_t C,
                              uint32_t fill_rgba, void* stream);

/*
 * Canvas pixels -> each frame's own pixels, in place.  boxes: [N, k, 4] (x1 y1 x2 y2) f32, 16-byte aligned, as the decode writes them
 * with normalize_boxes = 0; `table` as above.  With sx = float(new_w) / float(w) and sy = float(new_h) / float(h):
 * x' = (x - pad_left) / sx, y' = (y - pad_top) / sy, one rounding per operation; clip != 0 clamps to [0, w] / [0, h].
 * The axes have their own ratio because rounding new_h and new_w makes them differ slightly.
 */
int cnl_unletterbox_boxes_f32(float* boxes, const void* table, int32_t N, int32_t k, int32_t clip, void* stream);

/*
 * The same canvas from YUV 4:2:0 video surfaces (NV12, I420): colour conversion fused into the letterbox, so that no RGB frame is
 * ever written.  One launch for N frames of different sizes; the result is bit for bit cnl_letterbox_bilinear_u8 (C = 3) applied
 * to the frames converted by the rule below.
 *
 * `table` is a device array of N records, one per frame (or per tile: a tile is a window), 72 bytes each, 8-byte aligned:
 *     offset  0  const void* y, u, v      first byte of the Y plane and the first U and V samples (uint8, device memory)
 *     offset 24  int32 y_pitch, c_pitch   bytes from one row to the next in the Y plane / in the chroma plane(s)
 *     offset 32  int32 c_step             bytes from one chroma sample to the next: 2 with v = u + 1 for NV12 (interleaved UV), 1 for I420
 *     offset 36  int32 x0, y0             where the window starts in the frame (odd origins are legal)
 *     offset 44  int32 h, w               size of the window, >= 1 (the whole frame: x0 = y0 = 0 and the frame's size)
 *     offset 52  int32 new_h, new_w       size of the resized window inside the canvas, 1..height / 1..width
 *     offset 60  int32 pad_top, pad_left  where it starts: pad_top + new_h <= height, pad_left + new_w <= width
 *     offset 68  int32 reserved           0
 * The frame itself has even height and width; its chroma planes are half its size.  Window pixel (sy, sx) is Y byte
 * y[(y0 + sy) * y_pitch + x0 + sx] with the chroma sample at row (y0 + sy) >> 1, column (x0 + sx) >> 1 (nearest chroma: what OpenCV's
 * cvtColor(COLOR_YUV2RGB_NV12 / _I420) does).  The resize taps are clamped to the window, as cnl_letterbox_bilinear_u8 clamps to its frame.
 *
 * coef: six int32 in HOST memory, {y_off, CY, CVR, CVG, CUG, CUB}.  In 32-bit integers, >> an arithmetic shift, sat8 a clamp to 0..255:
 *     yy = max(0, Y - y_off) * CY + (1 << 19)
 *     R = sat8((yy + CVR * (V - 128)) >> 20),  G = sat8((yy + CVG * (V - 128) + CUG * (U - 128)) >> 20),  B = sat8((yy + CUB * (U - 128)) >> 20)
 * OpenCV's BT.601 limited-range constants are {16, 1220542, 1673527, -852492, -409993, 2116026}; the library knows no colour
 * standard, the host chooses the integers.  CNL_E_UNSUPPORTED for a set that could overflow 32 bits: y_off in 0..255, CY >= 0 and
 * 255 * CY + 2^19 + 128 * max(|CVR|, |CVG| + |CUG|, |CUB|) < 2^31 are required.
 *
 * out: [N, height, width, 3] RGB u8, height and width positive multiples of 32, 4-byte aligned; outside a window byte c of every pixel
 * is bits 8c..8c+7 of fill_rgba.  Every byte is written exactly once; a frame's result depends on its record only.  N = 0 is a no-op.
 */
typedef struct cnl_yuv420_frame {
    const void* y;
    const void* u;
    const void* v;
    int32_t y_pitch, c_pitch;
    int32_t c_step;
    int32_t x0, y0;
    int32_t h, w;
    int32_t new_h, new_w;
    int32_t pad_top, pad_left;
    int32_t reserved;
} cnl_yuv420_frame;
int cnl_letterbox_yuv420_u8(const void* table, uint8_t* out, int32_t N, int32_t height, int32_t width, const int32_t* coef,
                            uint32_t fill_rgba, void* stream);

/*
 * Detected objects cut out of their frames at one fixed size: boxes [N, k, 4] (x1 y1 x2 y2 f32 in each frame's own pixels, 16-byte
 * aligned, e.g. what cnl_unletterbox_boxes_f32 or cnl_merge_tiles_f32 left) -> out [N, k, crop_h, crop_w, C] u8.  Two launches on
 * `stream`, nothing goes to the host: a record kernel turns every slot (n, j) into one record of the frame's own type, and the gather
 * kernel of the two entry points above runs over those N * k records, so a crop is bit for bit what cnl_letterbox_bilinear_u8 gives for
 * the window sliced out of the frame (for YUV frames: out of the converted frame).
 *
 * frames: device array of N WHOLE-FRAME records.  coef == NULL: cnl_letterbox_frame records of C-channel frames.  coef != NULL:
 * cnl_yuv420_frame records with x0 = y0 = 0, coef being the six integers of cnl_letterbox_yuv420_u8 in host memory (same overflow
 * condition), and C must be 3.  Of a record only the pointers, strides / pitches and h, w (the frame's size H, W) are read.
 *
 * Live rule.  Slot (n, j) is live when (count == NULL or j < count[n]) and (scores == NULL or scores[n * k + j] >= score_threshold);
 * count: N int32, scores: [N, k] f32, both in device memory and optional.  A NaN score is not live.
 *
 * Window rule.  Every step is ONE fp32 operation (no fused multiply-add), so that numpy float32 reproduces it bit for bit:
 *     bw = x2 - x1, bh = y2 - y1
 *     xa = x1 - pad * bw, xb = x2 + pad * bw       (the product and the sum round separately; y alike with bh)
 *     x0 = (int)clamp(floorf(xa), 0, W), xe = (int)clamp(ceilf(xb), 0, W), w = xe - x0      (y alike with H)
 * with clamp(v, 0, L): t = v > 0 ? v : 0, then t < L ? t : L, in float before the conversion (a NaN becomes 0, +-1e30 stays in
 * range).  The slot is DEAD if it is not live, if any of x1 y1 x2 y2 is not finite, or if w < 1 or h < 1 (a box outside the frame,
 * an inverted box, x1 == x2 on an integer).  windows [N, k, 4] int32 (16-byte aligned) receives (x0, y0, w, h), (0, 0, 0, 0) for a
 * dead slot.
 *
 * Target.  keep_aspect == 0: the window is stretched to crop_h x crop_w.  keep_aspect != 0: the geometry rule of
 * cnl_letterbox_bilinear_u8 above on (h, w, crop_h, crop_w), evaluated on the device in double (two divisions, min, a multiply,
 * round half to even, clamped to 1..target), centred with the odd pixel at the bottom / right, the rest fill_rgba.  A dead slot's
 * crop is fill_rgba everywhere.  Every byte of `out` is written exactly once.
 *
 * records: workspace of N * k records of the frames' type (40 / 72 bytes each, 8-byte aligned); the library allocates nothing.
 * crop_w is a multiple of 4, >= 4 (112 x 112, 256 x 128, 128 x 64 are all fine); crop_h >= 1; a crop is smaller than 2 GiB; pad is
 * finite and >= 0; N, k >= 0 with N * k < 2^31 (above 65535 slots the gather is launched in chunks).  N == 0 or k == 0 is a no-op.
 */
int cnl_crop_boxes_u8(const void* frames, const float* boxes, const float* scores, float score_threshold, const int32_t* count, int32_t N,
                      int32_t k, int32_t C, const int32_t* coef, float pad, int32_t keep_aspect, void* records, int32_t* windows, uint8_t* out,
                      int32_t crop_h, int32_t crop_w, uint32_t fill_rgba, void* stream);

/*
 * Detections drawn onto their frames, in place: the output side of the frame pipeline (annotated preview, evidence clips, the
 * surface handed to an encoder).  boxes [N, k, 4] (x1 y1 x2 y2 f32 in each frame's own pixels, 16-byte aligned) and the frames as
 * cnl_crop_boxes_u8 takes them: `frames` is a device array of N WHOLE-FRAME records, of type cnl_letterbox_frame when yuv == 0 (C = 3
 * or 4 channels; channel 3 is never modified), of type cnl_yuv420_frame with x0 = y0 = 0 when yuv != 0 (C = 3).  Of a record only the pointers,
 * strides / pitches, c_step and h, w (the frame's size H, W <= 32768) are read.  Two launches on `stream` (a record kernel, one thread
 * per slot; a paint kernel over the tiles of a max_h x max_w frame, the largest of the batch: pixels of a frame beyond that size are
 * not painted), nothing goes to the host, no float atomics.  Everything below is integer once the corners are rounded.
 *
 * Colours.  The library knows no colour standard: palette is P + 1 four-byte entries in device memory (1 <= P <= 256), ALREADY in the
 * frames' own space, byte c of an entry = bits 8c..8c+7: R G B for packed frames, Y U V for YUV frames; entry P is text_color.  The
 * slot colour is palette[labels[n * k + j] mod P] with a non-negative modulus (labels: [N, k] int64, optional: entry 0 without).
 *
 * Live rule.  cnl_crop_boxes_u8's: slot (n, j) is live when (count == NULL or j < count[n]) and (scores == NULL or
 * scores[n * k + j] >= score_threshold).  A NaN score is not live.
 *
 * Corners.  For each coordinate, one fp32 operation per step: v = rintf(x) (round half to even); v = v > -32768 ? v : -32768;
 * v = v < 32767 ? v : 32767; then the conversion to int.  This gives X1, Y1, X2, Y2.  A slot is DEAD if it is not live, if any
 * coordinate is not finite, or if X2 < X1 or Y2 < Y1.  A box wholly outside the frame is live but paints nothing.
 *
 * Layers of a slot.  With t = thickness (1..32), o = (t - 1) / 2 in integer division, i = t - o:
 *     Interior  pixels with X1 <= x <= X2 and Y1 <= y <= Y2, painted only when fill_alpha = a > 0 (a in 0..256), per byte
 *               out = (old * (256 - a) + colour * a + 128) >> 8.
 *     Ring      pixels with X1 - o <= x <= X2 + o and Y1 - o <= y <= Y2 + o that are NOT in X1 + i <= x <= X2 - i and
 *               Y1 + i <= y <= Y2 - i, set to the slot colour: t pixels wide, with SQUARE corners (cv2.rectangle rounds the corners
 *               of thick lines; this rule does not).
 *     Tag       only when tag_scale = s > 0 (s in 0..8) and numbers[n * k + j] = m >= 0 (numbers: [N, k] int32, optional), d the
 *               count of m's decimal digits: a rectangle (6 d + 1) s wide and 9 s high, its left edge at X1 - o, its top at
 *               T = Y1 - o - 9 s, or at T = Y1 - o if that is negative (the tag moves inside the box).  For the tag pixel at offset
 *               (ty, tx): gy = ty / s - 1, gx = tx / s - 1, q = gx / 6, c = gx % 6 (integer division of non-negative values).  The
 *               pixel is text_color when 0 <= gy < 7, gx >= 0, q < d, c < 5 and bit (4 - c) of row gy of the glyph of the q-th most
 *               significant digit is set; otherwise the slot colour.  Glyph rows, top to bottom, five bits, the most significant
 *               the left column:
 *                   0: 01110 10001 10011 10101 11001 10001 01110      5: 11111 10000 11110 00001 00001 10001 01110
 *                   1: 00100 01100 00100 00100 00100 00100 01110      6: 00110 01000 10000 11110 10001 10001 01110
 *                   2: 01110 10001 00001 00010 00100 01000 11111      7: 11111 00001 00010 00100 01000 01000 01000
 *                   3: 11111 00010 00100 00010 00001 10001 01110      8: 01110 10001 10001 01110 10001 10001 01110
 *                   4: 00010 00110 01010 10010 11111 00010 00010      9: 01110 10001 10001 01111 00001 00010 01100
 *
 * Order.  A pixel's final value is the result of applying the slots j = k - 1 down to 0 (slot 0, the top score, ends on top); within
 * a slot interior, then ring, then tag.  Everything is clipped to the frame.  A byte that no layer of any slot covers keeps its
 * value: pitch padding and everything outside the h x w window of a surface included.
 *
 * YUV 4:2:0.  The Y plane follows the rule with byte 0 of the colours.  Chroma sample (cy, cx) is painted as if it were the pixel
 * (2 cy, 2 cx) (nearest chroma, as in cnl_letterbox_yuv420_u8) through the same layers in the same order with bytes 1 and 2 (U, V);
 * the blend is applied per plane.  Interleaved UV (c_step == 2, v == u + 1) and separate planes both go through c_step.
 *
 * records: workspace of N * k * 64 bytes, 16-byte aligned; the library allocates nothing.  N <= 65535, N * k < 2^31.  N == 0 or
 * k == 0 is a no-op.
 */
int cnl_draw_boxes_u8(const void* frames, const float* boxes, const int64_t* labels, const int32_t* numbers, const float* scores,
                      float score_threshold, const int32_t* count, int32_t N, int32_t k, int32_t C, int32_t yuv, const uint32_t* palette,
                      int32_t P, int32_t thickness, int32_t fill_alpha, int32_t tag_scale, int32_t max_h, int32_t max_w,
                      void* records, void* stream);

/*
 * The flip test (test-time augmentation of the original CenterNet): the network also sees every image mirrored left-right and the two
 * sets of head outputs are averaged BEFORE pseudo-NMS and top-k.  For a batch of N images the network runs on 2N inputs, input N + n
 * being input n mirrored AT THE NETWORK INPUT, x -> W_in - 1 - x.  W_in is a multiple of 32 and the output stride divides it, so input
 * column x maps to feature column W - 1 - x exactly.  The doubled batch is ONE forward, so both halves come from one plan and one
 * launch list, whatever the batch size.
 *
 * cnl_mirror_append_u8 builds the doubled uint8 input in one launch: src [N,H,W,C] and dst [2N,H,W,C] dense, C in 1..4,
 *     dst[n] = src[n],   dst[N + n, y, x] = src[n, y, W - 1 - x].
 * dst must not overlap src; 2 * N * H * W * C < 2^31; an empty batch is a no-op.  Any byte alignment (4-byte aligned pointers with
 * W * C % 4 == 0 move whole words).
 *
 * cnl_flip_merge_f32 merges up to three head maps of the 2N forward (logical shape [2N, C, H, W] each) in one launch.  The rule:
 *     merged[n, c, y, x] = 0.5f * ( a[n, c, y, x] + b[n, p(c), y, W - 1 - x] )
 * where a is the map of the first N inputs and b the map of the mirrored ones.  p(c) = c, except for a map with swap_lr != 0 (box_2d:
 * its channels are the distances left, top, right, bottom, and left and right trade places under a mirror; C must be 4), where p swaps
 * channels 0 and 2.  The arithmetic is one IEEE fp32 add followed by one multiply by 0.5, nothing fused: NaN and inf propagate as
 * they fall, denormals are kept, and the result equals (a + b.flip(-1)[:, perm]) * 0.5 in torch bit for bit.  The heatmap operand is
 * whatever map the caller has (post-sigmoid or logits); box_2d is averaged as the raw head output, before the decode's exp /
 * multiplier / clamp (with box_log the average of logarithms: a geometric mean of the sizes).
 *
 * `maps` is a HOST array of n_maps (0..3) descriptors, copied into the launch.  a, b and dst are device pointers, 4-byte aligned, each
 * addressed through its own element strides of the logical axes (n, c, y, x) as the decode does: element (n, c, y, x) of a lies at
 * a + n * a_sn + c * a_sc + y * a_sh + x * a_sw.  a and b are separate pointers, not one [2N] tensor: a forward that ran in
 * sub-batches may hand its halves over separately.  dst elements must be distinct and must not overlap a or b.  Channels-last maps
 * (every channel stride 1, C % 4 == 0) and plane maps (every column stride 1) move 16 bytes per access, everything else single
 * elements; no alignment beyond 4 bytes is asked for in either.  N * C * H * W < 2^31 per map.  N, H or W == 0, or n_maps == 0, is a
 * no-op.  No allocation, no synchronisation.
 */
typedef struct cnl_flip_map {
    const float* a;                    /* the map of inputs 0 .. N-1 */
    int64_t a_sn, a_sc, a_sh, a_sw;
    const float* b;                    /* the map of inputs N .. 2N-1 (the mirrored images) */
    int64_t b_sn, b_sc, b_sh, b_sw;
    float* dst;                        /* merged, logical [N, C, H, W] */
    int64_t d_sn, d_sc, d_sh, d_sw;
    int32_t C;
    int32_t swap_lr;                   /* != 0: channels 0 and 2 of b trade places (C == 4) */
} cnl_flip_map;                        /* 128 bytes */
int cnl_flip_merge_f32(const cnl_flip_map* maps, int32_t n_maps, int32_t N, int32_t H, int32_t W, void* stream);
int cnl_mirror_append_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

/*
 * Sliced inference, the merge: the decoded boxes of the V views (network-sized tiles cut out of a frame, plus optionally the whole
 * frame letterboxed) of N frames go back into each frame's own pixels, and the duplicates the tile overlaps create are removed by a
 * greedy non-maximum suppression per frame.  Three launches for the whole batch, no device synchronisation, no float atomics.  (The
 * tiles themselves are cnl_letterbox_bilinear_u8 records whose src points inside a frame, with new_h = h, new_w = w and no pads: a
 * 1:1 resize returns the source bytes.)
 *
 * boxes [V, k, 4] (x1 y1 x2 y2 in view pixels, 16-byte aligned), scores [V, k], labels [V, k] i64: what the decode writes for the V
 * views with normalize_boxes = 0.  frame_first_view: N + 1 int32 in device memory, non-decreasing, [0] = 0, [N] = V: frame n owns the
 * views frame_first_view[n] .. frame_first_view[n + 1] - 1.  `views` is a device array of V records, 32 bytes each, 4-byte aligned:
 *     offset  0  int32 frame_w, frame_h   the size of the frame the view was cut from
 *     offset  8  int32 x0, y0             where the view's window starts in the frame (0 for the full-frame view)
 *     offset 16  int32 pad_left, pad_top  the letterbox pads of the view (0 for a tile)
 *     offset 24  float sx, sy             view pixels per frame pixel: float(new_w) / float(w), float(new_h) / float(h) (1 for a tile)
 *
 * The rule, one rounding per operation (a numpy restatement reproduces it bit for bit):
 *   1. candidate c = v * k + r of a frame (v counted from the frame's first view) takes part if scores[c] > score_threshold (a NaN
 *      score never does; -0 and +0 are the same score);
 *   2. its box goes to the frame: x' = (x - pad_left) / sx + float(x0), y' = (y - pad_top) / sy + float(y0), then clamped to
 *      [0, frame_w] x [0, frame_h] as fminf(fmaxf(v, 0), limit): a NaN coordinate becomes 0 (no NaN reaches the match test);
 *   3. the frame's candidates are ordered by score descending, equal scores by c ascending;
 *   4. only the first max_candidates of that order take part (max_candidates in 1..16384);
 *   5. walking in order, candidate i is kept unless an already kept j matches it: (class_aware == 0 or label_j == label_i) and
 *      inter > match_threshold * denom, with iw = max(min(x2i, x2j) - max(x1i, x1j), 0), ih alike, inter = iw * ih,
 *      area = (x2 - x1) * (y2 - y1), denom = (area_i + area_j) - inter for metric 0 (IoU), min(area_i, area_j) for metric 1 (IoS: a
 *      box cut by a tile edge has a small IoU with the whole box from the neighbouring tile);
 *   6. the first K_out kept candidates of frame n, in order, are written to out_boxes [N, K_out, 4] (16-byte aligned), out_scores,
 *      out_labels (i64) and out_source [N, K_out] (the candidate number c, for gathering embeddings); out_count[n] says how many.
 *      Rows past the count hold score 0, label 0, box 0 and source -1: every output element is written.
 * A frame's output depends on that frame's views only, not on N or on the launch geometry.
 *
 * Limits (CNL_E_BAD_ARG otherwise): N in 0..65535, V >= 0, k >= 1, V * k <= 2^30, K_out >= 1, max_candidates in 1..16384, metric 0 or 1,
 * thresholds not NaN.  frame_first_view is read on the device and cannot be validated by the call: entries are forced into 0..V and a
 * decreasing pair gives an empty frame, so nothing is read or written out of bounds; but a table whose frames SHARE views is outside
 * the contract — the workspace is sized for disjoint frames, and a frame whose bit matrix would not fit in it is written as empty
 * (out_count 0, all padding).
 *
 * ws: cnl_merge_tiles_workspace_bytes(N, V, k, max_candidates) bytes of device memory, 256-byte aligned (0 is returned for sizes the
 * merge rejects).  N = 0 is a no-op; V = 0 writes N empty frames.
 */
size_t cnl_merge_tiles_workspace_bytes(int32_t N, int32_t V, int32_t k, int32_t max_candidates);
int cnl_merge_tiles_f32(const float* boxes, const float* scores, const int64_t* labels, const void* views,
                        const int32_t* frame_first_view, int32_t N, int32_t V, int32_t k, int32_t K_out, int32_t max_candidates,
                        float score_threshold, float match_threshold, int32_t metric, int32_t class_aware, float* out_boxes,
                        float* out_scores, int64_t* out_labels, int32_t* out_source, int32_t* out_count, void* ws, size_t ws_bytes,
                        void* stream);

/*
 * The soft merge: Gaussian / linear soft-NMS (Bodla et al., "Soft-NMS", 2017) over the views of a frame, the merge rule of the
 * original CenterNet's multi-scale test (every scale is one full-frame view).  A picked box does not delete its neighbours, it lowers
 * their scores, so the second of two real objects that overlap by more than the hard threshold survives with a smaller score.  The
 * reference has no soft-NMS to compare with: this comment is the specification and tests/soft_nms_ref.py restates it in numpy.
 * Two launches for the whole batch (the sort stage of cnl_merge_tiles_f32, then one workgroup per frame), no device synchronisation,
 * no float atomics.  Arguments, the `views` records, frame_first_view and the outputs are cnl_merge_tiles_f32's.
 *
 * The rule:
 *   1. The candidates of a frame are those of cnl_merge_tiles_f32, rules 1-4: score > score_threshold (a NaN score never), boxes
 *      mapped into the frame in fp32 and clamped, ordered by (score descending, candidate number ascending), the first max_candidates
 *      of that order (max_candidates in 1..4096 HERE: nine scales of 300 detections fit).  A candidate's index in that order is its
 *      POSITION.
 *   2. Every candidate has a WORKING SCORE, a float64, at first its fp32 score.  All float64 arithmetic below is one IEEE rounding per
 *      operation (no fused multiply-add); thresholds and sigma are the fp32 arguments widened.
 *   3. For r = 0, 1, ... while r < K_out: among the candidates not yet picked whose working score is > score_threshold take the one
 *      with the largest working score, among equal scores (-0 equals +0) the lowest position; if there is none, stop.
 *   4. The pick is output row r: its box, label, source (the candidate number c, as in cnl_merge_tiles_f32) and its working score
 *      rounded once to fp32.
 *   5. Every candidate not yet picked with the pick's label (class_aware == 0: every candidate not yet picked) has its working score
 *      multiplied by a weight w.  With the fp32 coordinates of the two boxes widened to float64:
 *          iw = max(min(x2p, x2c) - max(x1p, x1c), 0), ih alike, inter = iw * ih,
 *          ua = ((x2p - x1p) * (y2p - y1p) + (x2c - x1c) * (y2c - y1c)) - inter, ov = inter / ua;
 *      if ua > 0 is false (degenerate boxes) w = 1; otherwise
 *          method 2 (gaussian): w = exp(-(ov * ov) / sigma)   (exp is the platform's float64 exp: the one operation that is NOT
 *                               reproducible to the bit; scores agree with another platform's to a few float64 ulp per decay)
 *          method 1 (linear):   w = ov > iou_threshold ? 1 - ov : 1
 *          method 0 (hard):     w = 0 if the fp32, division-free predicate of cnl_merge_tiles_f32's rule 5 with metric 0 holds for
 *                               (pick, candidate) with match_threshold = iou_threshold, else 1.
 *      (inter = 0 gives w = 1 exactly for methods 1 and 2, whatever the thresholds.)
 *   6. Rows past the count hold score 0, label 0, box 0 and source -1; out_count[n] is the number of picks.  Every element is written.
 * Properties (proved on the restatement by tests/test_multiscale_host.py):
 *   - With scores >= 0 (what a sigmoid gives) working scores only decay, so the picks leave in non-increasing score order, and
 *     stopping at K_out equals "soft-NMS of every class to exhaustion, then the K_out best over all classes", the two steps of the
 *     original CenterNet.
 *   - Method 0 with score_threshold >= 0 is cnl_merge_tiles_f32 with metric 0 and the same thresholds, bit for bit (a removed
 *     candidate's working score is 0, which is not > score_threshold).
 *   - A frame's output depends on that frame's views only, not on N or on the launch geometry.
 *
 * Limits (CNL_E_BAD_ARG otherwise): those of cnl_merge_tiles_f32 with max_candidates in 1..4096; method 0, 1 or 2; sigma positive and
 * finite (whatever the method); thresholds not NaN.  ws: cnl_merge_soft_workspace_bytes(N, V, k, max_candidates) bytes, 256-byte
 * aligned: the sort keys and the sorted candidates, no bit matrix (cnl_merge_tiles_workspace_bytes is unchanged and always enough).
 */
size_t cnl_merge_soft_workspace_bytes(int32_t N, int32_t V, int32_t k, int32_t max_candidates);
int cnl_merge_soft_f32(const float* boxes, const float* scores, const int64_t* labels, const void* views,
                       const int32_t* frame_first_view, int32_t N, int32_t V, int32_t k, int32_t K_out, int32_t max_candidates,
                       float score_threshold, int32_t method, float sigma, float iou_threshold, int32_t class_aware, float* out_boxes,
                       float* out_scores, int64_t* out_labels, int32_t* out_source, int32_t* out_count, void* ws, size_t ws_bytes,
                       void* stream);

/*
 * COCO box evaluation (eval/coco.py: CocoEvaluator -> pycocotools COCOeval, iouType "bbox") without pycocotools and without the
 * detections leaving the device.  Two entry points (pure additions: the ABI number stays); both are asynchronous on `stream`, allocate
 * nothing and do no device synchronisation.
 *
 * The rule — COCOeval on the records CocoEvaluator.create_coco builds (eval/coco.py:78-107): every annotation has iscrowd = 0 and no
 * `ignore`, area = w * h, categories 0 .. num_classes-1, image ids in order of arrival.  tests/coco_eval_ref.py restates it in numpy;
 * every comparison with it is an equality of float64 bits.
 *   Parameters.  T: iouThrs = np.linspace(.5, .95, 10).  R: recThrs = np.linspace(0, 1, 101).  M: maxDets = (1, 10, 100).  A: the area
 *     ranges all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10]; a box is OUT of a range when area < lo or
 *     area > hi (both bounds inclusive: area 1024 is small and medium).
 *   Numbers.  All arithmetic is float64, every operation rounded on its own (no fused multiply-add; the division is the IEEE one).
 *     Detection boxes are fp32 x1 y1 x2 y2: w = x2 - x1 and h = y2 - y1 are formed in fp32 and then widened, x = x1, y = y1.  Ground
 *     truths are float64 x y w h as given.  Areas are the float64 products w * h.  Coordinates and scores must be finite.
 *   IoU of detection D and ground truth G: w = min(Dx + Dw, Gx + Gw) - max(Dx, Gx), h alike; IoU = 0 if w <= 0 or h <= 0; otherwise
 *     i = w * h, u = (Dw * Dh + Gw * Gh) - i, IoU = i / u.
 *   Per image and category: the detections of the category (slots below count[n]; a label outside 0..num_classes-1 is dropped) ordered
 *     by descending score, stably (equal scores keep their slot order); the first 100 are kept, a detection's place in that list is
 *     its CLASS RANK (0-based).
 *   Per (image, category, area range a, threshold t): a ground truth is IGNORED when its area is out of range a.  The detections are
 *     walked in class-rank order; for each one, with best = min(t, 1 - 1e-10): among the not yet taken, not ignored ground truths of
 *     the category with IoU >= best the largest IoU wins, the LAST in order of arrival among equals; only if there is none, the same
 *     choice among the not yet taken ignored ones.  A winner is taken; the detection is matched and inherits the winner's ignored
 *     flag.  (This is COCOeval's sequential walk over the ground truths sorted not-ignored first: tests/test_coco_eval_host.py checks
 *     the equivalence.)  An unmatched detection whose own area is out of range a is ignored.
 *   Accumulate, per (category c, range a, maxDet m): the detections of c with class rank < m, in order of arrival (image, then rank),
 *     ordered by descending score, stably.  npig = the not ignored ground truths of c in range a over all images.  npig == 0: the
 *     cell's precision and recall stay -1.  Otherwise per t: tp = cumsum(matched & ~ignored), fp = cumsum(~matched & ~ignored),
 *     rc = tp / npig, pr = tp / (fp + tp + 2^-52); recall[t, c, a, m] = rc[-1] (0 without detections); pr is made non-increasing from
 *     the right (pr[i-1] = max(pr[i-1], pr[i])); precision[t, r, c, a, m] = pr[first i with rc[i] >= R[r]], 0 when there is none.
 *   Summarise (host): AP = the mean of the entries > -1 of a precision slice, AR of a recall slice, -1 for a slice without any.
 *
 * cnl_coco_match_f64: one launch for a batch of N images, one workgroup per image.  boxes [N, k, 4] fp32 (16-byte aligned), scores
 * [N, k] fp32, labels [N, k] i64, count NULL or [N] i32 (the slots that hold detections; clamped to 0..k); gt_boxes [N, Gmax, 4] f64
 * x y w h, gt_labels [N, Gmax] i64 (a label outside 0..num_classes-1 takes no part), gt_count [N] i32 (clamped to 0..Gmax).  Written
 * for every detection slot: out_rank [N, k] i32 (the class rank; -1 for a dropped slot: past the count, label out of range, or rank
 * >= 100), out_matched and out_ignored [N, k] i64 (bit a * 10 + t of each; 0 for a dropped slot).  npig [num_classes, 4] i64 is
 * INCREMENTED (integer atomics): the caller zeroes it once per epoch.  A record depends on its own image only.
 * Limits (CNL_E_BAD_ARG otherwise): N in 0..2^20 (0 is a no-op), k in 1..1024, Gmax in 1..1024, num_classes in 1..2^20.
 *
 * cnl_coco_accumulate_f64: one launch per evaluation, one workgroup per (category, range, maxDet).  The caller has ordered the epoch's
 * `total` records (total < 2^31) by category, inside a category by descending score, equal scores in order of arrival (two stable
 * sorts), with the dropped records (rank -1) behind the last category: rank, matched, ignored are the match's outputs in that order,
 * and segment_first [num_classes + 1] i64 holds where each category's records start (entries are forced into 0..total on the
 * device).  npig as above.  Written, every element: precision [10, 101, num_classes, 4, 3] f64 and recall [10, num_classes, 4, 3] f64,
 * both dense with the last axis fastest.
 */
int cnl_coco_match_f64(const float* boxes, const float* scores, const int64_t* labels, const int32_t* count, const double* gt_boxes,
                       const int64_t* gt_labels, const int32_t* gt_count, int32_t N, int32_t k, int32_t Gmax, int32_t num_classes,
                       int32_t* out_rank, int64_t* out_matched, int64_t* out_ignored, int64_t* npig, void* stream);
int cnl_coco_accumulate_f64(const int32_t* rank, const int64_t* matched, const int64_t* ignored, const int64_t* segment_first,
                            const int64_t* npig, int64_t total, int32_t num_classes, double* precision, double* recall, void* stream);

/*
 * Multi-object-tracking evaluation (eval/mot_challenge.py: evaluate_mot_tracking_sequence -> TrackEval) without TrackEval: HOTA, CLEAR
 * and Identity for MotChallenge2DBox.  Entry points only (the ABI number stays); all are asynchronous on `stream`, allocate nothing and
 * do no device synchronisation; the workspace queries are pure host functions.
 *
 * The rule — TrackEval's HOTA, CLEAR and Identity on the data the reference's writer produces: every ground truth of class 1 with
 * confidence 1, every prediction with confidence 1, one class, so TrackEval's preprocessing removes nothing and only relabels the ids of
 * each side to 0..n-1 in ascending order of the original id (the caller does that).  The boxes are evaluated as given: no text round
 * trip, no +1.  TrackEval is not at hand to compare against: this text is the authority, tests/mot_eval_ref.py restates it in numpy +
 * scipy, and every comparison with it is an equality (integers, float64 bits).
 *   Numbers.  All arithmetic is float64, every operation rounded on its own (no fused multiply-add; the division is the IEEE one).
 *     eps = 2^-52.  Coordinates must be finite.  An id repeated inside one frame is an error (refused by the caller).
 *   Assignment.  scipy.optimize.linear_sum_assignment's, ties included (csrc/lsap_device.h).
 *   Similarity s of ground truth g and prediction d, both x y w h: x0 = x, y0 = y, x1 = x + w, y1 = y + h;
 *     iw = max(min(x1g, x1d) - max(x0g, x0d), 0), ih alike; I = iw * ih; area = (x1 - x0) * (y1 - y0) per box; U = (areag + aread) - I;
 *     s = 0 when either area <= eps or U <= eps, otherwise I / U.  A frame's matrix is [ground truths, predictions] in slot order.
 *   Counts.  gt_count[gid] / trk_count[tid]: the frames that hold the id.
 *   HOTA, alpha = np.arange(0.05, 0.99, 0.05) (19 float64 values, passed in).
 *     Pass 1, per frame in frame order: r_i = the sum of row i in ascending prediction slot, sequentially (from 0.0); c_j = the sum of
 *       column j in ascending ground-truth slot, sequentially; den = (c_j + r_i) - s; sim_iou = s / den where den > eps, else 0;
 *       potential[gid, tid] += sim_iou, a pair's contributions arriving in FRAME ORDER (a zero adds +0.0 and may be skipped).
 *     gas = potential / ((gt_count + trk_count) - potential).
 *     Pass 2, per frame: no ground truth: FP[a] += n_pred; no prediction: FN[a] += n_gt; otherwise the assignment on
 *       -(gas[gid, tid] * s); per alpha the matched pairs with s >= alpha - eps count: TP[a] += n, FN[a] += n_gt - n, FP[a] += n_pred - n,
 *       the frame's sum of their s (ascending ground-truth slot, sequentially, from 0.0) is added to LocA_sum[a] in frame order, and
 *       matches[a][gid, tid] += 1.
 *     Per alpha: AssA = sum(m * (m / max(1, (gt_count + trk_count) - m))) / max(1, TP), each row (ground-truth id) summed in ascending
 *       tracker id from 0.0, the rows then added in ascending ground-truth id from 0.0 (a zero adds +0.0 and may be skipped); AssRe with
 *       max(1, gt_count) and AssPr with max(1, trk_count) in place of the inner denominator, in the same order.
 *     Host: LocA = max(1e-10, LocA_sum) / max(1e-10, TP); DetRe = TP / max(1, TP + FN); DetPr = TP / max(1, TP + FP);
 *       DetA = TP / max(1, TP + FN + FP); HOTA = sqrt(DetA * AssA); OWTA = sqrt(DetRe * AssA).  A sequence without predictions:
 *       FN = n_gt_dets, LocA = 1, every other field 0; without ground truth: FP = n_pred_dets, LocA = 1 (the general rule gives the same).
 *   CLEAR, threshold 0.5, per sequence, frames strictly in order; state prev[gid] and prev_step[gid], both "none" at first.
 *     No ground truth in the frame: FP += n_pred, the state is NOT touched.  No prediction: FN += n_gt, the state is not touched.
 *     Otherwise score = 1000 * (tid == prev_step[gid]) + s, set to 0 where s < 0.5 - eps; the assignment on -score; the pairs with
 *     score > eps are KEPT.  IDSW += the kept pairs whose prev[gid] is set and differs from tid; matched_count[gid] += 1 for the kept;
 *     prev[gid] = tid for the kept; prev_step is cleared, then set for the kept; frag_count[gid] += 1 where prev_step was "none" before
 *     the frame and is set after it; TP += kept, FN += n_gt - kept, FP += n_pred - kept; MOTP_sum += the frame's sum of s over the kept
 *     pairs (ascending ground-truth slot, sequentially, from 0.0), in frame order.  At the end ratio = matched_count / gt_count over the
 *     ids (gt_count > 0); MT = #(ratio > 0.8); PT = #(ratio >= 0.2) - MT; ML = n_gt_ids - MT - PT; Frag = sum(frag_count - 1 over
 *     frag_count > 0); CLR_Frames = the number of frames.
 *     Host: MOTA = (TP - FP - IDSW) / max(1, TP + FN); MOTP = MOTP_sum / max(1, TP); MODA = (TP - FP) / max(1, TP + FN);
 *       CLR_Re = TP / max(1, TP + FN); CLR_Pr = TP / max(1, TP + FP); CLR_F1 = TP / max(1, TP + 0.5 * FN + 0.5 * FP);
 *       MTR, PTR, MLR = MT, PT, ML / max(1, MT + ML + PT); sMOTA = (MOTP_sum - FP - IDSW) / max(1, TP + FN);
 *       FP_per_frame = FP / max(1, CLR_Frames); MOTAL = (TP - FP - (log10(IDSW) if IDSW > 0 else IDSW)) / max(1, TP + FN).
 *       A sequence without predictions: CLR_FN = n_gt_dets, ML = n_gt_ids, MLR = 1, everything else 0 (CLR_Frames too) and no final
 *       fields; without ground truth: CLR_FP = n_pred_dets, MLR = 1, everything else 0.
 *   Identity, threshold 0.5: pm[gid, tid] = the frames with s >= 0.5.  With G ground-truth and T tracker ids, (G + T)^2 matrices:
 *     fn[i, :T] = gt_count[i] - pm[i, :], fn[i, T + i] = gt_count[i], fn[:G, T:] otherwise 1e10; fp[:G, j] = trk_count[j] - pm[:, j],
 *     fp[G + j, j] = trk_count[j], fp[G:, :T] otherwise 1e10; the rest 0.  One assignment on fn + fp; IDFN / IDFP = the sums of fn / fp
 *     over it (integers); IDTP = sum(gt_count) - IDFN; IDR = IDTP / max(1, IDTP + IDFN); IDP = IDTP / max(1, IDTP + IDFP);
 *     IDF1 = IDTP / max(1, IDTP + 0.5 * IDFP + 0.5 * IDFN).  Without predictions: IDFN = n_gt_dets and no final fields; without ground
 *     truth: IDFP = n_pred_dets.
 *   COMBINED_SEQ (host), TrackEval's rule: integer fields and the *_sum fields are summed over the sequences; AssA, AssRe, AssPr are
 *     averaged weighted by each sequence's HOTA_TP, per alpha: sum(x * TP) / max(1, sum(TP)), sequences in order of arrival;
 *     LocA = max(1e-10, sum(LocA * TP)) / max(1e-10, sum(TP)); then the final fields are recomputed.
 *
 * cnl_mot_tables: the pooled input of one evaluation (host struct of device pointers; every member is 8 bytes).  Frame f of F owns ground
 * truths gt_off[f] .. gt_off[f + 1], predictions pr_off[f] .. pr_off[f + 1] and the row-major [ng, np] matrix at sim_off[f]; frm_seq[f] is
 * its sequence.  Sequence s of S owns frames seq_frm[s] .. seq_frm[s + 1], ground-truth ids seq_gid[s] .. (G of them: gt_ids of its frames
 * are 0..G-1), tracker ids seq_tid[s] .. (T), the [G, T] pair block at seq_pair[s] and, for Identity, (G + T)^2 workspace entries at
 * seq_idm[s] (none where G + T > 1024).  gt_count [sum_g] / pr_count [sum_t]: the frames that hold each id.  The scalars repeat what
 * the tables say (pool sizes, the largest G, the largest frame sides and the largest ng * np); the device checks every offset it reads
 * against them and reports a contradiction as status 5 instead of indexing with it.
 * Limits: a frame holds at most 1024 objects on its smaller side and 4096 on its larger (CNL_E_UNSUPPORTED); S in 1..65535,
 * F < 2^26, n_gt, n_pr, sum_g, sum_t < 2^31, null or misaligned pointers, negative or contradictory sizes, a workspace smaller than
 * the query's answer: CNL_E_BAD_ARG, before anything touches the device.
 *
 * cnl_mot_similarity_f64: one launch writes every frame's matrix into sim [sim_total].
 * cnl_mot_hota_f64: sim as written above; alpha [19] f64 on the device.  Written: out_f64 [S, 4, 19] (LocA_sum, AssA, AssRe, AssPr),
 *   out_i64 [S, 3, 19] (TP, FN, FP), status [S] i32 (0, or the worst frame's: 1 a non-finite score, 2 infeasible, 3 too large, 5 tables).
 * cnl_mot_clear_f64: out_f64 [S] (MOTP_sum), out_i64 [S, 8] (TP, FN, FP, IDSW, MT, PT, ML, Frag), status [S]; one single-wave workgroup
 *   per sequence.
 * cnl_mot_identity_f64: pm [pair_total] i32 is written (zeroed, then counted with integer atomics); out_i64 [S, 2] (IDFN, IDFP);
 *   status [S]: 3 for a sequence with G + T > 1024, whose pm block is the input for solving that one assignment elsewhere.
 */
typedef struct cnl_mot_tables {
    const double* gt_boxes;      /* [n_gt, 4] x y w h */
    const double* pr_boxes;      /* [n_pr, 4] */
    const int32_t* gt_ids;       /* [n_gt] relabelled, per sequence */
    const int32_t* pr_ids;       /* [n_pr] */
    const int64_t* gt_off;       /* [F + 1] */
    const int64_t* pr_off;       /* [F + 1] */
    const int64_t* sim_off;      /* [F + 1] */
    const int32_t* frm_seq;      /* [F] */
    const int64_t* seq_frm;      /* [S + 1] */
    const int64_t* seq_gid;      /* [S + 1] */
    const int64_t* seq_tid;      /* [S + 1] */
    const int64_t* seq_pair;     /* [S + 1] */
    const int64_t* seq_idm;      /* [S + 1] */
    const int32_t* gt_count;     /* [sum_g] */
    const int32_t* pr_count;     /* [sum_t] */
    int64_t F, S, n_gt, n_pr, sim_total, pair_total, sum_g, sum_t, id_total;
    int64_t max_gids, max_gt_frame, max_pr_frame, max_frame_pairs;
} cnl_mot_tables;
int cnl_mot_similarity_f64(const cnl_mot_tables* tables, double* sim, void* stream);
int64_t cnl_mot_hota_workspace_bytes(const cnl_mot_tables* tables);
int cnl_mot_hota_f64(const cnl_mot_tables* tables, const double* sim, const double* alpha, double* out_f64, int64_t* out_i64,
                     int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
int64_t cnl_mot_clear_workspace_bytes(const cnl_mot_tables* tables);
int cnl_mot_clear_f64(const cnl_mot_tables* tables, const double* sim, double* out_f64, int64_t* out_i64, int32_t* status,
                      void* workspace, int64_t workspace_bytes, void* stream);
int64_t cnl_mot_identity_workspace_bytes(const cnl_mot_tables* tables);
int cnl_mot_identity_f64(const cnl_mot_tables* tables, const double* sim, int32_t* pm, int64_t* out_i64, int32_t* status,
                         void* workspace, int64_t workspace_bytes, void* stream);

/*
 * ResNet stem: Conv2d(3,64,7,stride=2,padding=3,bias=False)+BN+ReLU (torchvision resnet.conv1/bn1/relu).
 * x is read through explicit element strides (sn,sc,sh,sw) so NCHW-contiguous and channels_last
 * callers are both zero-copy (models/meta.py:97-98 precedent); y is NHWC [N, H/2, W/2, 64].
 * w: the PACKED weights that cnl_stem_pack_weights_f32 makes from the OHWI [64][7][7][3] (BN-folded) weights — LDS images copied
 * verbatim by LDS-DMA: the fp32 image [154][64] (row k = ky*22 + kx*3 + c; the 22nd row of every ky is zero) followed by the
 * scaled two-way fp16 split [piece][21 groups of 8 k][64][8] and its power-of-two scale (csrc/stem_f16x2.hip: the default kernel
 * forms each fp32 product on the fp16 matrix cores, input scaled per workgroup patch; algo = CNL_ALGO_F32 selects the fp32
 * matrix-core kernel); cnl_stem_packed_weight_floats() sizes the buffer; bias: [64].
 * y_absmax (all three stem entry points, ABI v10): NULL, or N * cnl_absmax_stride() floats zeroed by the caller on the stream — the fp16-split kernel folds max |y| of
 * image n into y_absmax[n * cnl_absmax_stride()] (atomic max on the bit pattern; the values are post-ReLU), the hand-over the first Winograd layer takes as
 * cnl_conv_params.x_absmax instead of a pass over the stem's output.  The fp32 kernel (CNL_ALGO_F32 without the fused pool) ignores it.
 */
size_t cnl_stem_packed_weight_floats(void);
int cnl_stem_pack_weights_f32(const float* w_ohwi, float* w_packed, void* stream);
int cnl_stem_conv7x7_f32(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                         const float* w, const float* bias, float* y, float* y_absmax,
                         int32_t N, int32_t H, int32_t W, uint32_t algo, void* stream);

/* The stem and resnet.maxpool in ONE launch: y = MaxPool2d(3, stride 2, padding 1)(ReLU(BN(conv7x7/2(x)))) as NHWC
 * [N, (Ho-1)/2+1, (Wo-1)/2+1, 64] with Ho = (H-1)/2+1, Wo = (W-1)/2+1; bit-identical to cnl_stem_conv7x7_f32 followed by
 * cnl_maxpool3x3s2_nhwc_f32 (always the fp16-split stem kernel), without the stride-2 feature map ever reaching memory.  The call
 * initialises y itself (stream-ordered: the cells that several workgroups merge are zeroed, every other cell is stored once).                                                                                         */
int cnl_stem_conv7x7_maxpool_f32(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                 const float* w, const float* bias, float* y, float* y_absmax,
                                 int32_t N, int32_t H, int32_t W, void* stream);

/* The stem on uint8 frames: x is [N, H, W, 3]-like uint8 addressed through BYTE strides (sn, sc, sh, sw); A.Normalize
 * — (float(x) - mean255[c]) * inv_std255[c], the arithmetic of cnl_normalize_u8_nhwc_f32, bit for bit — is applied to the staged patch
 * inside the kernel, so the fp32 image never exists in HBM (3 B/pixel read instead of 12 written + 12 read).  mean255 / inv_std255: HOST
 * arrays of 3 floats.  fuse_maxpool != 0: y is the pooled map of cnl_stem_conv7x7_maxpool_f32, else the conv output of
 * cnl_stem_conv7x7_f32.  Bit-identical to cnl_normalize_u8_nhwc_f32 followed by the fp32-input entry points (CNL_ALGO_AUTO).            */
int cnl_stem_conv7x7_u8(const uint8_t* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const float* mean255,
                        const float* inv_std255, const float* w, const float* bias, float* y, float* y_absmax, int32_t N, int32_t H, int32_t W,
                        int32_t fuse_maxpool, void* stream);

/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on NHWC (torchvision resnet.maxpool). C % 4 == 0. */
int cnl_maxpool3x3s2_nhwc_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                              void* stream);

/*
 * Fused decode = CenterNet.decode_detections (models/centernet.py:229-304)
 *              + EmbeddingHead.gather_at_indices (models/fairmot.py:63-73) when reid != null:
 *   3x3 (nms_kernel) max-pool pseudo-NMS with equality mask, per-pixel max/argmax over classes,
 *   per-image sorted top-k (ties: score desc, flat index asc), label / ltrb-box / embedding gather,
 *   box decode to x1y1x2y2.
 * heat/box/reid element (n,c,y,x) at n*s_n + c*s_c + y*s_h + x*s_w (elements): any NCHW or NHWC view.
 * Outputs: scores [N,k] f32, indices [N,k] i64 (flat y*W+x), labels [N,k] i64, boxes [N,k,4] f32,
 * emb [N,k,E] f32 (may be null when reid is null).  Exactly those N*k (x 4, x E) elements are written, each once.
 * Alignment: heat / box / reid and every output need the alignment of their element only (4 bytes; 8 for indices /
 * labels) — wider loads and stores are chosen per launch where the pointer, the strides and C / E allow them and never
 * change a result.  workspace: cnl_decode_workspace_bytes(N, H, W) bytes, 16-byte aligned (else CNL_E_BAD_ARG), no byte
 * beyond that size is touched.  The standalone gathers below: element alignment throughout.
 */
typedef struct cnl_decode_params {
    const float* heat; int64_t heat_sn, heat_sc, heat_sh, heat_sw;
    const float* box;  int64_t box_sn, box_sc, box_sh, box_sw;
    const float* reid; int64_t reid_sn, reid_sc, reid_sh, reid_sw;   /* reid may be null */
    int32_t N, C, H, W, E;
    int32_t k;               /* num_detections, 1 <= k <= min(1024, H*W)                              */
    int32_t nms_kernel;      /* odd, 1..7 (reference default 3, centernet.py:93)                      */
    int32_t normalize_boxes; /* !=0: divide by (W,H) (centernet.py:299-301) else multiply by stride    */
    int32_t box_log;         /* !=0: exp() the offsets first (centernet.py:283-284)                   */
    float box_multiplier;    /* centernet.py:285                                                      */
    float stride;            /* output stride (centernet.py:303), e.g. 4                              */
    float* scores; int64_t* indices; int64_t* labels; float* boxes; float* emb;
    void* workspace; size_t workspace_bytes;
} cnl_decode_params;

size_t cnl_decode_workspace_bytes(int32_t N, int32_t H, int32_t W);
int cnl_decode_f32(const cnl_decode_params* p, void* stream);
/* Which kernels cnl_decode_f32 runs for p (a pure host function, reporting only: the launcher itself calls the same decision; nothing is
 * launched and no pointer is dereferenced).  Returns what cnl_decode_f32 returns for the same arguments short of a HIP error; on CNL_OK
 * (each output may be null):
 *   *stage1  1 channel-minor (heat_sc == 1)   2 channel-minor with C % 8 == 0 (16-byte loads, strips of 16 or 4 rows)
 *            3 class planes (heat_sw == 1, W % 4 == 0, the other strides % 4 == 0, 16-byte aligned, C >= 4)   4 generic (any strides)
 *   *vec     floats per load of stage 1: 4 / 2 / 1 for the channel-minor kernel — the widest that divides C and the n / y / x strides
 *            at a base pointer aligned to it; 4 for kernels 2 and 3, 1 for the generic one
 *   *strip   rows of the map per workgroup
 *   *topk    where the top-k keeps an image's score keys: 0 sixteen registers per thread (H*W <= 16384), 1 LDS (<= 24576),
 *            2 forty-eight registers (<= 49152 and H*W % 4 == 0), 3 their upper halves in LDS (<= 49152), 4 memory only.
 * Every combination computes the same bytes for finite heat values.
 * NON-FINITE VALUES in image n's heat, box or reid leave image n's own outputs unspecified and never change another image's outputs.
 * Whatever the values: image n's indices lie in [0, H*W) and are pairwise distinct, its labels lie in [0, C), and all N*k (x 4, x E)
 * output elements are written once — the gathers and crops behind the decode stay inside their buffers — and the top-k terminates (it
 * orders unsigned integer keys: every bit pattern, NaN included, has one; a positive NaN sorts above +inf, a negative one below -inf).
 * What is NOT the same in every combination is which class a pixel keeps when NaN stands beside other values: each stage-1 kernel gives a
 * thread its own subset of the classes, takes the subset's first class unconditionally and a later one only if it compares greater
 * (never, with a NaN on either side), and merges the subsets by another comparison; and heat * mask is NaN for a +-inf that is no peak
 * (tests/test_gpu_nonfinite.py: NaN, +-inf and a mix of them in one image of three, every stage-1 kernel and key storage).                */
int cnl_decode_forms(const cnl_decode_params* p, int32_t* stage1, int32_t* vec, int32_t* strip, int32_t* topk);

/*
 * Standalone gathers at caller-supplied flat indices [N,k] (i64), for the Gen-A per-head calls
 * heads["box_2d"].gather_at_indices / EmbeddingHead.gather_at_indices (models/fairmot.py:141-143, 63-73;
 * arithmetic of CenterNet.gather_and_decode_boxes, models/centernet.py:263-304).  Strides in elements.
 */
int cnl_gather_boxes_f32(const float* box, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const int64_t* indices,
                         float* boxes, int32_t N, int32_t H, int32_t W, int32_t k, int32_t normalize_boxes,
                         int32_t box_log, float box_multiplier, float stride, void* stream);
int cnl_gather_embeddings_f32(const float* reid, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                              const int64_t* indices, float* emb, int32_t N, int32_t E, int32_t H, int32_t W,
                              int32_t k, void* stream);

/*
 * All-gather record (replaces the pickled all_gather_object of eval/coco.py:10-18):
 * rec[n][j][0:4] = box, [4] = score, [5] = bit pattern of (int32)label, [6:6+E] = embedding.  E may be 0 (emb null).  Every pointer
 * needs its element's alignment only (4 bytes; 8 for labels).
 */
int cnl_pack_detections_f32(const float* boxes, const float* scores, const int64_t* labels, const float* emb,
                            float* rec, int32_t N, int32_t k, int32_t E, void* stream);
int cnl_unpack_detections_f32(const float* rec, float* boxes, float* scores, int64_t* labels, float* emb,
                              int32_t N, int32_t k, int32_t E, void* stream);

/*
 * SURVEY.md §8f next #3 — the remaining neck options of make_upsample / make_conv (models/layers.py:40-101).
 *
 * cnl_deconv2x_nhwc_f32: upsample_type="conv_transpose" = nn.ConvTranspose2d(C, C', K, stride=2, padding=(K + K%2)/2 - 1,
 * output_padding=K%2, bias=False) + BatchNorm2d + ReLU (layers.py:86-93; K = deconv_kernel in {2,3,4}; output is exactly
 * 2H x 2W).  Computed as FOUR sub-pixel phase convolutions on the MFMA implicit-GEMM kernel (no zero-stuffing): phase
 * (dy,dx) writes y[n, 2i+dy, 2j+dx, :].  y = act(deconv(x) + bias) (+ residual at the same 2x position, added after the
 * activation: Fuse's "in1 + resize(in2)", layers.py:160-174).
 * `w` is the PACKED weight: for phase ph = 2*dy + dx a block [Cout][KHp][KWp][Cin] (OHWI), blocks back to back, where with
 * (taps, pad) = cnl_deconv_phase_geometry(K, d) per axis and p = (K + K%2)/2 - 1:
 *     w_packed[ph][co][jy][jx][ci] = scale[co] * W[ci][co][dy + p + 2*(pad_y - jy)][dx + p + 2*(pad_x - jx)]
 * (W = ConvTranspose2d.weight [Cin][Cout][K][K]; scale = folded BN gamma/sqrt(var+eps)); cnl_deconv_weight_floats() = K*K*Cin*Cout.
 */
typedef struct cnl_deconv_params {
    const float* x;         /* input  [N, H_in, W_in, ldx]                         */
    const float* w;         /* packed phase weights (see above)                    */
    const float* bias;      /* [Cout]                                              */
    const float* residual;  /* null, or [N, 2H_in, 2W_in, ldr]                     */
    float* y;               /* output [N, 2H_in, 2W_in, ldy]                       */
    int32_t N, H_in, W_in, Cin, Cout, K;
    int32_t ldx, ldy, ldr;
    uint32_t flags;         /* CNL_RELU | CNL_RELU6                                */
} cnl_deconv_params;
int cnl_deconv2x_nhwc_f32(const cnl_deconv_params* p, void* stream);
int cnl_deconv_phase_geometry(int32_t K, int32_t d, int32_t* taps, int32_t* pad);
size_t cnl_deconv_weight_floats(int32_t Cin, int32_t Cout, int32_t K);

/*
 * nn.Upsample(scale_factor=2, mode="nearest" | "bilinear") (layers.py:99; bilinear = align_corners=False) on NHWC, optionally
 * adding `residual` at the output resolution (Fuse: in1 + resize(in2)).  mode: 0 = nearest, 1 = bilinear.  C % 4 == 0.
 * Nearest feeding a "normal" conv never needs this (CNL_UPSAMPLE_IN folds it into the conv); it exists for bilinear and for
 * the depthwise path.
 */
int cnl_upsample2x_nhwc_f32(const float* x, const float* residual, float* y, int32_t N, int32_t H_in, int32_t W_in, int32_t C,
                            int32_t ldx, int32_t ldr, int32_t ldy, int32_t mode, void* stream);

/* The sum of a general Fuse node (reference models/layers.py:160-175; nodes with three inputs and/or resize="down" — BiFPN's bottom-up
 * path — and weighted_fusion with any resize):
 *     y = (g0 * in0 [+ g1 * in1] + gl * resize(last)) / den          in1 == NULL for a two-input node
 * in0 / in1 / y are [N, H, W, C] NHWC with pixel strides ld0 / ld1 / ldy; `last` is resized on the fly by `mode`:
 *   0  nn.Upsample(2, "nearest")   last is [N, H/2, W/2, C]       1  nn.Upsample(2, "bilinear", align_corners=False)   same shape
 *   2  nn.MaxPool2d(2, 2)          last is [N, 2H, 2W, C]         3  none (already resized, e.g. by cnl_deconv2x_nhwc_f32)
 * Unweighted fusion: g* = den = 1 (bit-exact plain sum); weighted (layers.py:164-167): g_j = relu(w_j), den = sum_j relu(w_j) + 1e-6.
 * C and the strides multiples of 4, pointers 16-byte aligned.  HBM-bound: reads each input once, writes y once. */
int cnl_fuse_sum_nhwc_f32(const float* in0, const float* in1, const float* last, float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                          int32_t ld0, int32_t ld1, int32_t ldl, int32_t ldy, float g0, float g1, float gl, float den, int32_t mode,
                          void* stream);

/*
 * conv_type="separable", depthwise half (layers.py:58-62): nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False) + BN + ReLU6.
 * w: [3][3][C] (tap-major, BN scale folded), bias [C]; flags: CNL_RELU | CNL_RELU6.  C % 4 == 0.  The pointwise half is
 * cnl_conv2d_nhwc_f32 (1x1) with CNL_RELU6.
 */
int cnl_depthwise3x3_nhwc_f32(const float* x, const float* w, const float* bias, float* y, int32_t N, int32_t H, int32_t W,
                              int32_t C, int32_t ldx, int32_t ldy, uint32_t flags, void* stream);

/*
 * conv_type="deformable" (layers.py:9-38, 47-54): DeformableConv2dBlock = offset_conv (+ sigmoid mask_conv for version 2) feeding
 * torchvision DeformConv2d(K x K, stride 1, padding (K-1)/2, bias=False), then BN + ReLU.  Here: offsets and mask logits come from
 * ONE ordinary K x K conv (cnl_conv2d_nhwc_f32, Cout = 2KK [+ KK], weights concatenated); this entry point does the deformable
 * sampling   col[n,y,x,k,:] = sigmoid(mask_k) . bilinear(x[n], y - p + ky + dy_k, x - p + kx + dx_k)   (torchvision's rule: zero
 * outside (-1,H) x (-1,W), corners outside the image contribute zero; offsets (dy, dx) interleaved per tap k = ky*K + kx);
 * the product with the [Cout][K*K*C] weight (OHWI order, BN folded) is a 1x1 cnl_conv2d_nhwc_f32 over col (pixel stride K*K*C).
 * om: [N,H,W,ldo] with channels [0, 2KK) offsets, [2KK, 3KK) mask logits (has_mask != 0).  C % 4 == 0.
 */
int cnl_deform_sample_nhwc_f32(const float* x, const float* om, float* col, int32_t N, int32_t H, int32_t W, int32_t C,
                               int32_t ldx, int32_t ldo, int32_t K, int32_t has_mask, void* stream);

/*
 * Step after the path for the tracking task: association costs of one frame against the current
 * track table, and the track-table update, so that per-frame embeddings never leave HBM — only the n x T cost matrices go to
 * the host for the Hungarian step (scipy, as in the reference) and the match list comes back.
 *
 * cnl_track_costs_f32 replaces models/tracker.py:133-137 (mask = scores >= detection_threshold; boolean-mask compaction),
 * :150 (scipy cdist "cosine", float64) and :162 (utils/box.py:84-92 box_iou_distance_matrix / box_giou_distance_matrix, float32):
 *   det_emb [k,E], det_box [k,4] x1y1x2y2, det_score [k] (k <= 1024); trk_emb [T,E], trk_box [T,4] (T may be 0);
 *   box_cost: 0 = none, 1 = "iou", 2 = "giou";
 *   n_det [1] <- number of detections with score >= threshold; det_index [k] <- their original indices, ascending (first n_det);
 *   reid_cost [n_det,T] f64 and box_cost_out [n_det,T] f32 <- row r is detection det_index[r] (dense, row stride T).
 * cnl_track_apply_f32 replaces Track.__init__ / Track.update_matched (models/tracker.py:228, 305-321, use_kalman=False) and the
 * list rebuild of :186-196 for the device-resident table: new row r is
 *   src_trk[r] >= 0, src_det[r] <  0 : old row src_trk[r] unchanged
 *   src_trk[r] >= 0, src_det[r] >= 0 : emb = (1-s)*old + s*e/|e|, box = det_box[src_det[r]]   (e = det_emb[src_det[r]])
 *   src_trk[r] <  0, src_det[r] >= 0 : emb = e/|e|,               box = det_box[src_det[r]]   (new track)
 * src_trk / src_det are device int32 arrays of T_new entries; new_emb/new_box must not alias the old table.
 * Alignment (the cost entries, cnl_track_frame_f32 and cnl_track_streams_f32), for a launch with tracks (T > 0; R > 0): det_box and trk_box
 * 16-byte aligned when box_cost != 0, det_emb and trk_emb 16-byte aligned when E % 4 == 0 (boxes and embedding rows are then read 16 bytes
 * at a time), else CNL_E_BAD_ARG; every other pointer, the outputs
 * n_det / det_index / reid_cost / box_cost_out and all of cnl_track_apply_f32's included, needs its element's alignment only.  Of
 * det_index only the first n_det entries and of the cost matrices only the n_det x T part are written.
 */
int cnl_track_costs_f32(const float* det_emb, const float* det_box, const float* det_score, int32_t k, int32_t E,
                        float detection_threshold, const float* trk_emb, const float* trk_box, int32_t T, int32_t box_cost,
                        int32_t* n_det, int32_t* det_index, double* reid_cost, float* box_cost_out, void* stream);
/* the same with the re-ID metric as an argument (models/tracker.py:51, 150: any scipy cdist metric): 0 "cosine", 1 "euclidean",
 * 2 "sqeuclidean", 3 "cityblock", 4 "chebyshev", 5 "canberra", 6 "braycurtis", 7 "correlation" (round 6: rows centred by their float64 mean in numpy's
 * pairwise order, then the cosine kernel) — each in float64 in scipy's operation order (bit for bit scipy's matrix; cosine / correlation to 1e-12).  Other metrics / callables: host fallback in tracker.py (opt-in). */
int cnl_track_costs_metric_f32(const float* det_emb, const float* det_box, const float* det_score, int32_t k, int32_t E,
                               float detection_threshold, const float* trk_emb, const float* trk_box, int32_t T, int32_t box_cost,
                               int32_t reid_metric, int32_t* n_det, int32_t* det_index, double* reid_cost, float* box_cost_out, void* stream);
/*
 * One frame's association in ONE launch and ONE record, so that the host makes a single stream synchronisation per frame and no
 * copy: the same compaction and costs as cnl_track_costs_metric_f32, written as
 *   int32 header[8] = { n, k, T, with_detections, off_index, off_dets, off_reid, off_box }   (byte offsets into the record)
 *   int32 det_index[k]                      at off_index  (first n valid)
 *   f32 boxes[k][4], f32 scores[k], int32 labels[k]   at off_dets   (only with_detections != 0: the frame's detections as the host-side
 *                                            track life cycle reads them, models/tracker.py:171-186; det_label read as label_kind says:
 *                                            1 int64, 2 int32, 3 float32; 0 = no labels, zeros)
 *   f64 reid_cost[n][T]                     at off_reid
 *   f32 box_cost[n][T]                      at off_box = off_reid + 8 n T   (box_cost != 0)
 * The kernel packs the matrices by the n it finds itself: the host needs no copy of the scores before the launch.  `record` holds
 * at least cnl_track_frame_bytes(k, T, with_detections) bytes (the n = k worst case; only the n x T part is written), is 8-byte
 * aligned and may be device memory or page-locked host memory from cnl_host_alloc — then the record crosses PCIe as the kernel's own
 * stores (52 KB for 58 x 70 pairs) and no copy-engine operation sits between the launch and the host's wait.
 */
int64_t cnl_track_frame_bytes(int32_t k, int32_t T, int32_t with_detections);
int cnl_track_frame_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                        int32_t k, int32_t E, float detection_threshold, const float* trk_emb, const float* trk_box, int32_t T,
                        int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record, int64_t record_bytes, void* stream);
/* src_trk / src_det may also be cnl_host_alloc memory (2 x T_new int32 read over PCIe by the kernel: no host -> device copy) */
int cnl_track_apply_f32(const float* trk_emb, const float* trk_box, const float* det_emb, const float* det_box,
                        const int32_t* src_trk, const int32_t* src_det, int32_t T_new, int32_t E, double smoothing,
                        float* new_emb, float* new_box, void* stream);

/*
 * Many video streams per step, assignment on the device (csrc/track_streams.hip).  The unit of work is ONE FRAME FROM EACH of S_live
 * streams: the association of every stream, Hungarian step included, in one pass of two back-to-back launches on `stream`; the host
 * synchronises once and reads the match lists.  No cost matrix crosses PCIe.
 *
 * Batched rectangular assignment: B independent problems in one launch, one single-wave workgroup each.  Problem b is the n_rows[b] x n_cols[b]
 * float64 matrix at cost + cost_offset[b] (elements) with row stride row_stride[b] >= n_cols[b]; all five arrays are device memory.
 * col4row + col4row_offset[b] receives n_rows[b] int32: the column assigned to each row, or -1 (rows > cols).  The result is EXACTLY
 * scipy.optimize.linear_sum_assignment's, ties included (same algorithm, order and float64 arithmetic: rectangular shortest augmenting
 * path, transposed when rows > cols).  status[b]: 0 ok; 1 a NaN or -inf entry; 2 infeasible (scipy raises ValueError in both cases);
 * 3 larger than max_rows x max_cols (or a negative size / row_stride < cols) — nothing is written to col4row unless the status is 0.
 * max_rows / max_cols bound every problem of the launch and size the workgroup's LDS (12 B per min-side row + 28 B per max-side column):
 * min(max_rows, max_cols) <= 1024 and max(max_rows, max_cols) <= 4096, else CNL_E_UNSUPPORTED.
 */
int cnl_lsap_batch_f64(const double* cost, const int64_t* cost_offset, const int32_t* row_stride, const int32_t* n_rows, const int32_t* n_cols,
                       int32_t B, int32_t max_rows, int32_t max_cols, int32_t* col4row, const int64_t* col4row_offset, int32_t* status,
                       void* stream);
/*
 * One association pass for S streams.  This step's detections of the S_live <= S participating streams are det_emb [S_live,k,E],
 * det_box [S_live,k,4], det_score [S_live,k], det_label [S_live,k] (label_kind as cnl_track_frame_f32): slot i belongs to stream live[i]
 * (int32, distinct, 0 <= live[i] < S).  ONE pooled track table trk_emb [R,E], trk_box [R,4]: stream s owns rows trk_off[s] .. trk_off[s+1]
 * (int32 [S+1], ascending, trk_off[S] <= R; no stream has more than T_max <= 4096 rows).  live and trk_off may be cnl_host_alloc memory.
 * Per live stream, what the single-stream path does between cnl_track_frame_f32 and cnl_track_apply_f32:
 *   1. compaction score >= detection_threshold and the n x T cost matrices (re-ID float64, box float32) by the device code of
 *      cnl_track_frame_f32 (bit-identical matrices), into the workspace;
 *   2. stage 1: assignment on the re-ID matrix, pairs with cost < reid_threshold kept (float64 compare);
 *   3. stage 2 (box_cost != 0): assignment on the box-cost sub-matrix of the still-unmatched detections x still-unmatched tracks (both
 *      ascending; converted to float64 as scipy does), pairs with cost < box_threshold kept (float32 compare);
 *   4. the stream's record at record + live[i] * record_stride (8-byte aligned; cnl_host_alloc memory or device memory):
 *        int32 header[16] = { n, k, T, status, off_index, off_dets, off_match, off_udet, off_utrk, n_match, n_match_stage1, n_udet,
 *                             n_utrk, with_detections, slot i, stream }        (byte offsets into the record)
 *        int32 det_index[k]                                at off_index  (first n valid: original indices of the kept detections)
 *        f32 boxes[k][4], f32 scores[k], int32 labels[k]   at off_dets   (with_detections != 0 only)
 *        int32 matches[n_match][2] = (detection row, track)   at off_match: stage 1 in row order, then stage 2 in row order — the order
 *                                                             tracker.py's match_with_threshold yields; rows index det_index, tracks the stream's rows
 *        int32 unmatched detection rows[n_udet], ascending  at off_udet;   int32 unmatched tracks[n_utrk], ascending  at off_utrk
 *      status: 0 ok; 1 / 2 / 3 as cnl_lsap_batch_f64 for stage 1, 17 / 18 / 19 for stage 2; 4 trk_off inconsistent with R.  With a status
 *      set the lists are not valid (a non-finite cost, e.g. a zero embedding under "cosine": scipy raises there — the caller redoes that
 *      stream through the single-stream path).
 * workspace, record and record_stride are 8-byte aligned (CNL_E_BAD_ARG otherwise); between the records of a larger record_stride, in the
 * records of streams that are not in `live`, and past workspace_bytes nothing is written.
 * cnl_track_streams_record_bytes(k, T_max, with_detections) is the smallest record_stride; cnl_track_streams_workspace_bytes(S, k, T_max)
 * bounds the device workspace (20 bytes per pair of the pooled table, k * R pairs, R <= S * T_max, plus the index lists); the sections of
 * stream s start at k * trk_off[s] pairs.
 * The table update needs no new kernel: cnl_track_apply_f32 does the pooled update when the index lists are global — src_trk[r] = row of
 * the OLD pooled table, src_det[r] = i * k + d for detection d of slot i, T_new = total rows of all streams; a stream that takes no part in
 * the step keeps its rows (src_det = -1).
 */
int64_t cnl_track_streams_workspace_bytes(int32_t S, int32_t k, int32_t T_max);
int64_t cnl_track_streams_record_bytes(int32_t k, int32_t T_max, int32_t with_detections);
int cnl_track_streams_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                          int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                          double reid_threshold, float box_threshold, const float* trk_emb, const float* trk_box, const int32_t* trk_off,
                          int32_t R, int32_t T_max, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* workspace,
                          int64_t workspace_bytes, void* record, int64_t record_stride, void* stream);

/*
 * BYTE low-score association (Zhang et al., ByteTrack), opt-in: one more association stage that keeps a track alive through an occlusion.
 * The entries below are the ones above with the stage added; without it (the entries above) nothing changes.
 * The rule, for scores s[0..k) compared in float32 as the compaction above does (a NaN score belongs to neither set):
 *   H = { d : s[d] >= detection_threshold } ascending (unchanged);  L = { d : low_threshold <= s[d] < detection_threshold } ascending.
 *   Stages 1 (re-ID) and 2 (box cost) run on H exactly as above: same matrices bit for bit, same matches in the same order.
 *   Stage 3: U = the tracks still unmatched after stage 2, ascending, restricted to the eligible ones (the caller's choice: e.g. the tracks
 *   that are ACTIVE at the start of the step, or all).  The cost is the configured box cost (box_cost 1 / 2, float32, the device function of
 *   stage 2) between the boxes of L and the table's track boxes; the |L| x |U| sub-matrix, converted to float64 as scipy does, is assigned
 *   as scipy.optimize.linear_sum_assignment does, and the pairs with cost < low_box_threshold are kept (float32 compare, as in stage 2).
 *   If L or U is empty the stage does nothing.
 *   A stage-3 pair (low detection d, track t): the track takes the box of detection d (d is the ORIGINAL index) — an ordinary measurement for
 *   its Kalman filter (cnl_track_kalman_f64 unchanged, src_det = d) — and its embedding row is carried over UNCHANGED: an occluded
 *   detection's appearance is not trusted.  Only tracks unmatched after all three stages count as unmatched; new tracks come from the
 *   unmatched members of H only, unmatched members of L are dropped.
 * Deviations from ByteTrack: unconfirmed tracks take part in stages 1 and 2 as in the reference (no separate unconfirmed pass); no score
 * fusion; the cost is this tracker's box cost on the table's boxes (the filtered ones with a Kalman filter), not a predicted box's.
 *
 * cnl_track_frame_low_f32: cnl_track_frame_f32 plus low_threshold.  The record is that entry's behind a larger header, with two sections
 * more (every section the old record holds carries the same values):
 *   int32 header[12] = { n, k, T, with_detections, off_index, off_dets, off_reid, off_box, n_low, off_low_index, off_low_box, 0 }
 *   int32 low_index[k]      at off_low_index = off_box + 4 n T   (first n_low valid: the original indices of L)
 *   f32 low_box[n_low][T]   at off_low_box = off_low_index + 4 k: row x is detection low_index[x] against every track
 * cnl_track_frame_low_bytes(k, T, with_detections) bounds the record (n + n_low <= k).  box_cost == 0, or a low_threshold outside
 * [0, detection_threshold] (a NaN included), is CNL_E_BAD_ARG; the other checks are cnl_track_frame_f32's.  Stage 3 itself is the host's.
 */
int64_t cnl_track_frame_low_bytes(int32_t k, int32_t T, int32_t with_detections);
int cnl_track_frame_low_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                            int32_t k, int32_t E, float detection_threshold, float low_threshold, const float* trk_emb, const float* trk_box,
                            int32_t T, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record, int64_t record_bytes,
                            void* stream);
/*
 * cnl_track_streams_low_f32: cnl_track_streams_f32 plus low_threshold, low_box_threshold and trk_eligible — one byte per row of the pooled
 * table (R bytes, device or cnl_host_alloc memory; non-zero = the row may be matched in stage 3; null = every row).  The cost launch
 * compacts L beside H and writes the |L| x T box costs into a further workspace section; the assign kernel runs stage 3 behind stage 2 with
 * the same solver and the same LDS bound (n_low <= k, |U| <= T_max).  The stream's record:
 *   int32 header[24]: fields 0..15 as cnl_track_streams_f32's, except that off_utrk / n_utrk list the tracks unmatched after ALL THREE
 *                     stages; 16 n_low, 17 n_low_match, 18 off_low_index, 19 off_low_match, 20..23 zero
 *   the sections of cnl_track_streams_f32's record (behind the 96-byte header), then
 *   int32 low_index[k]                     at off_low_index  (first n_low valid: the original indices of L)
 *   int32 low_matches[n_low_match][2] = (low row, track)   at off_low_match, in low-row order; low rows index low_index
 * status: as cnl_track_streams_f32, and 33 / 34 / 35 for stage 3 (1 / 2 / 3 of cnl_lsap_batch_f64: e.g. a NaN coordinate in a low detection).
 * cnl_track_streams_low_record_bytes / cnl_track_streams_low_workspace_bytes are the sizes (each at least the plain entry's); alignment,
 * the bytes left untouched (between records, past workspace_bytes, in the records of streams not in `live`) and the argument checks are
 * cnl_track_streams_f32's; box_cost == 0 or a low_threshold outside [0, detection_threshold] is CNL_E_BAD_ARG.
 */
int64_t cnl_track_streams_low_workspace_bytes(int32_t S, int32_t k, int32_t T_max);
int64_t cnl_track_streams_low_record_bytes(int32_t k, int32_t T_max, int32_t with_detections);
int cnl_track_streams_low_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                              int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                              double reid_threshold, float box_threshold, float low_threshold, float low_box_threshold, const float* trk_emb,
                              const float* trk_box, const int32_t* trk_off, const uint8_t* trk_eligible, int32_t R, int32_t T_max,
                              int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* workspace, int64_t workspace_bytes,
                              void* record, int64_t record_stride, void* stream);
/*
 * cnl_track_apply_keep_f32: cnl_track_apply_f32 plus keep_emb [T_new] (one byte per new row; device or cnl_host_alloc memory): a row with
 * src_trk[r] >= 0, src_det[r] >= 0 and keep_emb[r] != 0 takes the OLD row's embedding bytes and the detection's box (a stage-3 match).  A null
 * keep_emb, or all zeros, gives exactly cnl_track_apply_f32's output.
 */
int cnl_track_apply_keep_f32(const float* trk_emb, const float* trk_box, const float* det_emb, const float* det_box, const int32_t* src_trk,
                             const int32_t* src_det, int32_t T_new, int32_t E, double smoothing, float* new_emb, float* new_box,
                             const uint8_t* keep_emb, void* stream);

/*
 * The per-track Kalman filter on the device (csrc/track_kalman.hip): Track.__init__ / predict / update of models/tracker.py:243-262,
 * 281-290, 317-323 with use_kalman=True, for the rows of the device track table.  ONE launch behind cnl_track_apply_f32, driven by the same
 * two index lists, builds the new state tables (ping-pong, not in place):
 *   x [T_old,8] f64, P [T_old,64] f64 (row-major 8x8): the old tables; both null when there is no old table (then every row is a birth);
 *   det_box [*,4] f32, src_trk / src_det [T_new] int32: the operands cnl_track_apply_f32 was given (the lists may be cnl_host_alloc memory);
 *   flags [T_new] int32 (may be cnl_host_alloc memory): bit 0 = predict this row at the end;
 *   new_x [T_new,8], new_P [T_new,64] f64 <- the new tables; new_box [T_new,4] f32: the box table cnl_track_apply_f32 has just written;
 *   out_box [T_new,4] f64, out_status [T_new] int32: device memory or cnl_host_alloc memory (cnl_track_kalman_out_bytes(T_new) = 36 T_new
 *   holds both, out_box first).
 * Per new row r, with t = src_trk[r], d = src_det[r]:
 *   birth   (t <  0, d >= 0): b = det_box[d] converted to f64; x = (b, 0, 0, 0, 0); w = b2 - b0, h = b3 - b1; P = diag(s_i * s_i) with
 *                             s_i = (i odd ? h : w) / 10 for i < 4 and / 16 for i >= 4.  new_box[r] = float32(x[:4]), out_box[r] = x[:4].
 *   matched (t >= 0, d >= 0): old row t, the measurement update below with z = det_box[d]; new_box[r] = float32(x[:4]), out_box[r] = x[:4].
 *   carried (t >= 0, d <  0): old row t; new_box[r] is NOT written (it keeps the last updated box, not the predicted one: the reference's
 *                             behaviour); out_box[r] = x[:4].
 *   then, if bit 0 of flags[r] is set, the prediction step below; then new_x[r] / new_P[r] are stored; out_status[r] is always written.
 * Arithmetic: float64 throughout, one rounding per operation, no fused multiply-add, every sum starts with its first term and adds the others in
 * ascending index order; P is read and kept as its upper triangle and stored mirrored, so the stored matrix is exactly symmetric.  With
 * P = [[A, B], [B', C]] (4x4 blocks), F = [[I, I], [0, I]], H = [I 0]:
 *   update:  w = x2 - x0, h = x3 - x1, r_i = t_i * t_i with t_i = (i odd ? h : w) / 20 (i < 4);  y_i = z_i - x_i;
 *            S = A + diag(r) (only the diagonal is added to) = L D L' without square roots, column j = 0..3:
 *              c_ij = S_ij - sum_{k<j} c_ik * L_jk  (i = j..3; no subtraction for j = 0),  d_j = c_jj,  L_ij = c_ij / d_j  (i > j);
 *            K = P[:, :4] S^-1 row by row (m = 0..7):  u_i = P_mi - sum_{k<i} L_ik * u_k  (i = 0..3),  v_i = u_i / d_i,
 *              K_mi = v_i - sum_{k>i} L_ki * K_mk  (i = 3..0);
 *            x_m <- x_m + sum_{k<4} K_mk * y_k;
 *            P <- (I - KH) P (I - KH)' + K R K':  W_ij = P_ij - sum_{k<4} K_ik * P_kj,
 *              P_ij <- (W_ij - sum_{k<4} W_ik * K_jk) + sum_{k<4} (K_ik * r_k) * K_jk   for i <= j, mirrored.
 *   predict: w, h from x before the step; x_i <- x_i + x_{i+4} (i < 4);  A_ij <- (A_ij + B_ji) + (B_ij + C_ij) for i <= j, mirrored;
 *            B_ij <- B_ij + C_ij;  then P_ii <- P_ii + q_i * q_i with q_i = (i odd ? h : w) / 20 for i < 4 and / 160 for i >= 4.
 * The ONE deviation from the host path (BoxKalman, whose np.linalg.inv raises LinAlgError on a singular S): if a pivot d_j is not finite
 * and strictly positive — a zero-area box, or a non-finite state — the row skips the update: x and P stay as loaded and bit 0 of
 * out_status[r] is set.  Bit 1 marks a row without a source (t >= 0 without old tables, or t < 0 and d < 0: a caller's error): it is stored
 * as zeros.  Rows are independent: a non-finite row never changes another row's bits.  No atomics, no memset; the same bytes on every run.
 * CNL_E_BAD_ARG before any HIP call: T_new < 0; a null pointer other than x / P (which are null together); a new table that aliases the old
 * one; x, P, new_x, new_P or out_box not 8-byte aligned; det_box not 16-byte aligned (a box is read as one 16-byte word).  T_new == 0 returns
 * CNL_OK without a launch.
 */
int64_t cnl_track_kalman_out_bytes(int32_t T_new);
int cnl_track_kalman_f64(const double* x, const double* P, const float* det_box, const int32_t* src_trk, const int32_t* src_det,
                         const int32_t* flags, int32_t T_new, double* new_x, double* new_P, float* new_box, double* out_box,
                         int32_t* out_status, void* stream);

/*
 * Class-aware and Kalman-gated association, opt-in: the cost stage of the two association paths with gates inside the per-pair cost functions.
 * The entries above are unchanged; the assignment code is unchanged too — it solves the gated matrices, and the thresholds reject gated pairs.
 *
 * A gated pair's cost is the constant CNL_TRACK_GATE_COST = 1e5 (exact in float32 and float64; DeepSORT's INFTY_COST).  It is finite on purpose:
 * with +inf, scipy.optimize.linear_sum_assignment raises "cost matrix is infeasible" as soon as one class has more detections than tracks.  An
 * optimal assignment of the gated matrix restricted to the ungated pairs is the assignment of each class on its own, and every threshold below
 * 1e5 drops the gated pairs it had to use; so every threshold (re-ID, box, low box, motion_gate) >= 1e5 is CNL_E_BAD_ARG while a gate is on.
 *
 * Class gate (trk_label set): detection d and track row t may be matched only if label(d) == trk_label[t], label(d) being det_label[d] read by
 * label_kind and cast to int32 exactly as the record's label section is (label_kind 0: every label is 0).  A cross-class pair costs
 * CNL_TRACK_GATE_COST in the re-ID matrix, in the box matrix and in the low-score stage's box matrix.
 *
 * Motion gate (kx / kP set: the state tables cnl_track_kalman_f64 wrote, i.e. the PREDICTED state the previous step left), stage 1 only — the
 * box matrices are not motion-gated, as in DeepSORT.  For kept detection d with box z (float32 converted to float64) and track row t, in
 * float64, one rounding per operation, no fused multiply-add, every sum starting with its first term and adding the others in ascending order:
 *   1. x = kx[t][0:4], A = the upper-left 4 x 4 block of kP[t], read as its upper triangle;
 *   2. w = x2 - x0, h = x3 - x1, r_i = q_i * q_i with q_i = (i odd ? h : w) / 20;
 *   3. S = A + diag(r) = L D L' exactly as the update step of cnl_track_kalman_f64 factors it (one device function, shared);
 *   4. y_i = z_i - x_i;  u_i = y_i - sum_{k<i} L_ik * u_k  (i = 0..3; no subtraction for i = 0);  v_i = u_i / d_i;
 *      m = ((v0 * u0 + v1 * u1) + v2 * u2) + v3 * u3   — the squared Mahalanobis distance y' S^-1 y;
 *   5. a pivot d_j that is not finite and strictly positive, or an m for which m <= motion_gate is false (a NaN included), gates the pair:
 *      its re-ID cost is CNL_TRACK_GATE_COST.  Otherwise the re-ID cost is reid (its bits untouched) when motion_weight == 1, else
 *      (motion_weight * reid) + ((1 - motion_weight) * m)  (FairMOT's lambda; 1 - motion_weight is one float64 subtraction).
 * A cross-class pair is gated whatever its motion.  Pairs are independent: a NaN coordinate gates its own pairs and changes no other pair's bits.
 *
 * cnl_track_gate carries the operands (40 bytes); a null `gate`, or null members, switch that gate off.  trk_label [T] (pooled [R] for the
 * streams entry), kx [T,8] / kP [T,64] f64 (pooled likewise) are device or cnl_host_alloc memory.
 *
 * cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32: cnl_track_frame_low_f32 / cnl_track_streams_low_f32 plus `gate`.  Records,
 * workspace, sizes (the _low_ helpers), status words and checks are those entries'; "no low-score stage" is low_threshold ==
 * detection_threshold (n_low = 0), and then box_cost may be 0.  With every gate off they write byte for byte what the _low_ entries write.
 * CNL_E_BAD_ARG in addition: kx and kP not null together or not 8-byte aligned; trk_label not 4-byte aligned; with the motion gate, det_box
 * not 16-byte aligned (a box is read as one 16-byte word), motion_gate not in [0, 1e5) or motion_weight not in [0, 1] (a NaN included); with
 * any gate on, a threshold >= 1e5.  The class gate is on exactly when trk_label is set, so a caller whose table is empty (T == 0, R == 0: no
 * pairs) may pass null; with label_kind 0 every detection is of class 0.
 */
#define CNL_TRACK_GATE_COST 1e5
typedef struct cnl_track_gate {
    const int32_t* trk_label;   /* the tracks' labels (the label at birth); null: the class gate is off */
    const double* kx;           /* filter state table; null together with kP: the motion gate is off */
    const double* kP;
    double motion_gate;         /* threshold on m; DeepSORT's chi2inv95[4] is 9.4877 */
    double motion_weight;       /* 1: the re-ID cost as it is inside the gate */
} cnl_track_gate;
int cnl_track_frame_gated_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                              int32_t k, int32_t E, float detection_threshold, float low_threshold, const float* trk_emb, const float* trk_box,
                              int32_t T, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record, int64_t record_bytes,
                              const cnl_track_gate* gate, void* stream);
int cnl_track_streams_gated_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                int32_t S, int32_t S_live, const int32_t* live, int32_t k, int32_t E, float detection_threshold,
                                double reid_threshold, float box_threshold, float low_threshold, float low_box_threshold, const float* trk_emb,
                                const float* trk_box, const int32_t* trk_off, const uint8_t* trk_eligible, int32_t R, int32_t T_max,
                                int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* workspace, int64_t workspace_bytes,
                                void* record, int64_t record_stride, const cnl_track_gate* gate, void* stream);

/*
 * The track life cycle of a step over S streams on the device (csrc/track_lifecycle.hip), opt-in: what the host does between the records of
 * cnl_track_streams_f32 / _low_f32 / _gated_f32 and the table update (models/tracker.py:164-196, 305-347), so that a step is a fixed sequence
 * of launches without a synchronisation.  The entries above are unchanged and are given the CAPACITIES: every stream owns at most max_tracks
 * rows, the pooled tables and every per-row array below have C = S * max_tracks rows, R = C, T_max = max_tracks, T_new = C, and their records
 * (with_detections = 0), trk_off, trk_eligible, index lists and cnl_track_gate.trk_label are the device memory named here.
 *
 * Per-row state (cnl_track_rows, C rows; rows trk_off[s] .. trk_off[s+1] are stream s's, rows from trk_off[S] on are padding and zero):
 * track_id int64; state int32 (1 UNCONFIRMED, 2 ACTIVE, 3 INACTIVE); birth_age, inactive_age, label int32; box f64 [C,4], the REPORTED box;
 * trk_off int32 [S+1].  old_rows is read, new_rows written (ping-pong, never aliased).  next_track_id int64 [S] is updated in place.
 *
 * cnl_track_lifecycle_i32, queued behind the assign launch, two kernels:
 *  1. per stream s (one single-wave workgroup each), with i = slot_of[s] (int32 [S]: the slot of this step's detections, -1 no part):
 *     s == reset_stream (by value; -1: none): the stream is left with no rows and next_track_id[s] = 0, whatever its slot.
 *     -1, or a record whose status is not 0 (a SKIPPED stream — the stated deviation from the host path, which redoes such a stream on the host
 *         and raises scipy's error: here nothing can be read): the rows are carried, nothing ages, nothing predicts (flags 0).  A record whose
 *         k or section offsets do not fit record_stride (not one the association entry wrote with these sizes) is skipped likewise, code 4.
 *     else, from the stream's record: a stage-1/2 match (row, track) updates the track from detection POSITION `row` of slot i (the reference's
 *         quirk: not det_index[row]), a stage-3 match (low row x, track) from detection low_index[x] with keep_emb = 1; every other track is
 *         unmatched.  matched: UNCONFIRMED -> birth_age + 1, ACTIVE once birth_age >= min_birth_age; INACTIVE -> ACTIVE, inactive_age = 0.
 *         unmatched: UNCONFIRMED -> deleted; ACTIVE -> INACTIVE, inactive_age = 0; INACTIVE -> inactive_age + 1, deleted once inactive_age >=
 *         max_inactive_age.  The new rows are the surviving old rows in order, then one birth per unmatched detection row q (ascending) from
 *         detection det_index[q]: id = next_track_id[s]++, UNCONFIRMED, ages 0, the detection's label (read by label_kind as the record's label
 *         section is).  Capacity: only the first max_tracks - survivors births happen; the others are dropped and consume no id.
 *     status int32 [S][2], sticky (the caller clears it): word 0 = the first skipped step's association status in bits 0..15, bit 16 = births
 *     were dropped; word 1 = the `step` of the first event.
 *  2. the prefix sum of the streams' new counts -> new_rows.trk_off; the per-row state in pooled order; src_trk / src_det (global: slot * k + d)
 *     / keep_emb / flags (1 for the rows of a stream that took part, else 0) for cnl_track_apply_keep_f32 and cnl_track_kalman_f64 over C rows;
 *     trk_eligible[r] = the new row is ACTIVE (the next step's stage 3).  A padding row r carries itself: src_trk = r, src_det = -1, flag 0.
 * cnl_track_lifecycle_emit_f64, queued behind the table update and the filter, one kernel: new_rows.box[r] = a born / matched row's detection
 * box (kalman_box[r], the filter launch's out_box, when kalman_box is set), a carried row's old_rows.box[src_trk[r]]; and for each slot i < S_live
 * the ACTIVE rows of stream live[i] in row order: out_box [S_live, max_tracks, 4] (f32, or f64 with out_box_f64), out_track_id / out_label
 * [S_live, max_tracks] int64, out_count [S_live] int32; entries at and beyond the count are zero.
 * No allocation, no synchronisation, no atomics; the same bits on every run.  workspace: cnl_track_lifecycle_workspace_bytes, 8-byte aligned.
 * CNL_E_BAD_ARG before any HIP call: a null or misaligned pointer (int64 / f64 arrays, record, record_stride and workspace 8 bytes, the others
 * their element's), aliased old / new rows, a workspace too small, S / S_live / k / max_tracks out of range, a bad label_kind; CNL_E_UNSUPPORTED:
 * max_tracks > 4096 (the assignment's limit), S > 4096, S_live * k >= 2^31.
 */
typedef struct cnl_track_rows {
    int64_t* track_id;
    int32_t* state;
    int32_t* birth_age;
    int32_t* inactive_age;
    int32_t* label;
    double* box;
    int32_t* trk_off;
} cnl_track_rows;
typedef struct cnl_track_lifecycle {
    cnl_track_rows old_rows, new_rows;
    const void* record;         /* the association entry's records, device memory */
    int64_t record_stride;
    const int32_t* live;        /* [S_live] slot -> stream, as given to the association entry */
    const int32_t* slot_of;     /* [S] stream -> slot, -1, -2 */
    const void* det_label;      /* this step's detections, as given to the association entry */
    const float* det_box;
    int64_t* next_track_id;
    int32_t* status;
    int32_t* src_trk;           /* [C] each: the lists of the table update and the filter */
    int32_t* src_det;
    int32_t* flags;
    uint8_t* keep_emb;
    uint8_t* trk_eligible;
    const double* kalman_box;   /* emit: out_box of the filter launch [C,4]; null without a filter */
    void* out_box;              /* emit: the step's outputs */
    int64_t* out_track_id;
    int64_t* out_label;
    int32_t* out_count;
    void* workspace;
    int64_t workspace_bytes;
    int32_t S, S_live, k, max_tracks;
    int32_t label_kind, low_record;     /* low_record: the records have the _low layout */
    int32_t min_birth_age, max_inactive_age;
    int32_t step, out_box_f64;
    int32_t reset_stream, reserved;     /* reset_stream: a stream to forget in this call, -1 none */
} cnl_track_lifecycle;
int64_t cnl_track_lifecycle_workspace_bytes(int32_t S, int32_t max_tracks);
int cnl_track_lifecycle_i32(const cnl_track_lifecycle* p, void* stream);
int cnl_track_lifecycle_emit_f64(const cnl_track_lifecycle* p, void* stream);

/*
 * Camera-motion compensation, part 2 (csrc/track_lifecycle.hip): the global image shift of a step applied to the resident bank, ONE launch in
 * front of the step's association launch.  For each slot i < S_live with s = live[i] and (dx, dy) = shift[2i], shift[2i+1] (float32, in the units
 * of the boxes the bank is given), every row r of trk_off[s] .. trk_off[s+1] — all states — gets (dx, dy, dx, dy) added to trk_box[4r ..] (one
 * fp32 add each), to box[4r ..], the float64 reported box a carried row hands to the next emit (one float64 add of (double)dx / dy each), and,
 * when kx is not null, to kx[8r .. 8r+3], the positions of the filter state (likewise).  P, the velocities, embeddings, ages and ids are not
 * touched; rows of other streams are not touched.  A shift with a non-finite component SKIPS its stream and sets bit 17 of the stream's sticky
 * status word (status[2s], with status[2s+1] = step if the word was 0: the words of cnl_track_lifecycle_i32).  Offsets that do not lie in
 * 0 <= trk_off[s] <= trk_off[s+1] <= S * max_tracks, or a stream index outside 0 .. S-1, skip the slot.  `live` must not name a stream twice.
 * CNL_E_BAD_ARG before any HIP call: a null pointer (kx may be null), S, S_live or max_tracks out of range, trk_box / shift / live / trk_off /
 * status not 4-byte aligned, box / kx not 8-byte aligned.
 */
int cnl_track_shift_f64(float* trk_box, double* box, double* kx, const int32_t* trk_off, const int32_t* live, const float* shift, int32_t* status,
                        int32_t S, int32_t S_live, int32_t max_tracks, int32_t step, void* stream);

/*
 * Camera-motion compensation, part 1 (csrc/camera_motion.hip): the global translation between each stream's previous and current frame, by
 * block matching on a coarse luma plane.  Integer arithmetic throughout; tests/camera_motion_ref.py restates the rule in numpy and is held
 * equal to it.  Three launches, chosen by `stages` (bit 0 coarse luma, bit 1 block search, bit 2 aggregate; 7 is the whole call):
 *
 * Frames: L records (device memory).  src is a packed frame of `step` = 3 or 4 bytes per pixel (R, G, B first; a fourth byte is ignored) or,
 * with step = 1, a luma plane (the Y plane of an NV12 / I420 surface); h x w pixels, rows row_stride bytes apart, read in place and only read.
 *   luma:    step 1: the byte.  step 3 / 4: Y = (77 R + 150 G + 29 B + 128) >> 8.
 *   coarse:  d = downscale in {1, 2, 4, 8}; Hc = h / d, Wc = w / d (integer division: leftover rows and columns are dropped);
 *            coarse[y][x] = (sum of the d x d lumas + (d * d) / 2) >> (2 log2 d)   ((d * d) / 2 is 0 at d = 1), one byte, written densely
 *            (rows Wc bytes apart) to the record's `cur` plane.  `prev` is the plane the previous call wrote for the same stream at the same
 *            frame size, or null: no previous frame (status bit 0), and nothing is searched.
 *   blocks:  B = block in {8, 16}, R = radius in 1 .. 8, a grid of gy x gx blocks, each of 1 .. 16.  Along an axis of coarse length n with
 *            m blocks, block i starts at R + (i * (n - 2R - B)) / (m - 1), or at R + (n - 2R - B) / 2 when m == 1.  When Hc < 2R + B or
 *            Wc < 2R + B the frame is too small (status bit 2), and nothing is searched.
 *   search:  the shift s = (sx, sy) means cur(p) = prev(p - s): the content moved by s.  For every s in [-R, R]^2,
 *            SAD(s) = sum over the block of |cur[y0+y][x0+x] - prev[y0+y-sy][x0+x-sx]|; the winner has the smallest key
 *            (SAD, |sy| + |sx|, sy, sx) in lexicographic order.
 *   abstain: a block does not vote when it is flat: sum |cur - m| < min_texture * B * B with m = (sum cur + B * B / 2) / (B * B); or matches
 *            badly: best SAD > max_sad * B * B; or its centre pixel (cx, cy) = ((x0 + B / 2) * d, (y0 + B / 2) * d) lies inside a live box:
 *            x1 <= cx < x2 and y1 <= cy < y2 in float32 for some j < k with j < count[i] (count null: every j) whose four coordinates are
 *            finite (boxes [L, k, 4] x1 y1 x2 y2 in frame pixels; null: no mask).
 *   outputs of the search, per slot and block (row-major over the grid): vectors int16 (sx, sy) and sad int32 = the winner and its SAD;
 *            (0, 0) and -1 for a block that abstained or was not searched.
 *   aggregate: over the n blocks with sad >= 0: used = n; n < min_blocks: shift (0, 0) and status bit 1.  Otherwise sx* is the element at index
 *            (n - 1) / 2 of the ascending sx values, sy* likewise and independently, and shift = ((float)(sx* * d), (float)(sy* * d)), in the
 *            frame's own pixels.  status = bit 0 | bit 1 | bit 2 as above (an unsearched slot has n = 0, so bit 1 as well).
 * No atomics, no floats before the final conversion, no synchronisation; every word has one writer.
 * CNL_E_BAD_ARG before any HIP call: a null pointer (boxes and count may be null; count without boxes is refused), L < 1, k < 0 (k >= 1 with
 * boxes), a parameter outside the ranges above, min_texture / max_sad outside 0 .. 255, min_blocks < 1, stages outside 1 .. 7, shift / used / sad
 * / status / boxes / count not 4-byte aligned, vectors not 2-byte aligned, frames not 8-byte aligned.  CNL_E_UNSUPPORTED: L > 65535.
 */
typedef struct cnl_motion_frame {      /* 40 bytes */
    const void* src;
    void* cur;                          /* Hc * Wc bytes, written by stage bit 0 */
    const void* prev;                   /* Hc * Wc bytes, or null */
    int32_t h, w, row_stride, reserved;
} cnl_motion_frame;
typedef struct cnl_camera_motion {     /* 112 bytes */
    const cnl_motion_frame* frames;     /* [L], device memory */
    const float* boxes;                 /* [L, k, 4] or null */
    const int32_t* count;               /* [L] or null */
    float* shift;                       /* [L, 2] (dx, dy) */
    int32_t* used;                      /* [L] */
    int16_t* vectors;                   /* [L, gy * gx, 2] */
    int32_t* sad;                       /* [L, gy * gx] */
    int32_t* status;                    /* [L] */
    int32_t L, k, step, downscale;
    int32_t gy, gx, block, radius;
    int32_t min_texture, max_sad, min_blocks, reserved;
} cnl_camera_motion;
int cnl_camera_motion_u8(const cnl_camera_motion* p, int32_t stages, void* stream);

/*
 * Zone occupancy, line crossings and dwell events from the outputs of a device life-cycle step (csrc/track_zones.hip): ONE launch behind
 * cnl_track_lifecycle_emit_f64, no synchronisation.  tests/zones_ref.py restates the rule in numpy and is held equal to it bit for bit: all
 * geometry is float64 on the widened inputs, one rounding per operation, no contraction.
 *
 * Inputs, for L slots of M rows: boxes [L, M, 4] x1 y1 x2 y2 (float32, or float64 with boxes_f64), track_ids / labels [L, M] int64, count [L]
 * int32 (clamped to 0 .. M).  live int32 [S]: live[i], i < L, is slot i's stream; live[L ..] are the streams that take no part.  `live` names
 * every stream once; a slot whose stream index lies outside 0 .. S-1 is skipped.
 * Geometry, S records of 8 + 336 Z + 104 Ln bytes, device memory, only read: int32 n_zones, n_lines; Z zone records { int32 n_vertices (0: a
 * padding zone, nothing is inside it), dwell_alert, n_labels (0: every label), reserved; int64 labels[8]; double v[16][2] }; Ln line records
 * { double ax, ay, bx, by; int32 n_labels, reserved; int64 labels[8] } of which the first n_lines count.
 *
 *  1. anchor: anchor = 0 (bottom centre): ((x1 + x2) * 0.5, y2); 1 (centre): ((x1 + x2) * 0.5, (y1 + y2) * 0.5).  A row at or beyond count, or
 *     with a non-finite anchor, is NOT PRESENT this step; the latter sets status bit 0.
 *  2. zone membership, even-odd, no division: for every edge (xi, yi) -> (xj, yj), j the next vertex cyclically, with (yi > py) != (yj > py):
 *     t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi); toggle when yj > yi ? t > 0 : t < 0.  A track whose label is not among the zone's
 *     labels is outside it.
 *  3. line crossing of the segment p0 (the remembered anchor) -> p1 (this step's): cross(u, v) = u.x * v.y - u.y * v.x; d0 = cross(B - A,
 *     p0 - A) > 0, d1 likewise for p1; none if d0 == d1.  e0 = cross(p1 - p0, A - p0) > 0, e1 likewise for B; none if e0 == e1.  Otherwise
 *     forward (kind 3) if d1 — the track entered the side where cross > 0, on a y-down screen the right-hand side of A -> B —, backward (kind
 *     4) if not.  The line itself belongs to the side cross <= 0: a touch from that side and back counts nothing (from the other side: one
 *     backward and one forward crossing, net zero); a crossing through the shared endpoint of a polyline A-B, B-C counts once.  A track
 *     with no remembered anchor, or with a filtered label, crosses nothing.
 *  4. identity: per stream a list of at most E = 2 * max_tracks entries { id, anchor, inside mask, Z dwell counts, absent age }.  A present row
 *     takes the state of the FIRST entry with its id; none: it is new.  (Ids are distinct within a stream's step, as the bank's are; were
 *     they not, every such row takes that first entry.)  An entry no present row took is absent: age + 1; it is in no occupancy, its dwell
 *     stands, it makes no event; when age > max_absent it is forgotten with one exit event per zone it was inside.  When it returns, lines
 *     are tested from its remembered anchor and its dwell continues.  The new list: the present rows in row order (age 0), then the remembered
 *     absent entries in their previous order; entries beyond E are dropped without events: status bit 1.
 *  5. per present row and zone z: inside -> dwell = (was inside ? previous dwell : 0) + 1, else 0.  Events (track_id, kind, index, value):
 *     kind 1 enter zone (value 1: the track is new to the counter, else 0), 2 exit zone (value: the dwell it had), 3 / 4 forward / backward
 *     crossing of line `index` (value 0), 5 dwell reached exactly dwell_alert[z] > 0 (value: the dwell).  Order: the present rows in row
 *     order; per row the zones ascending (exit or enter, then the alert), then the lines ascending; then the expired entries in previous-list
 *     order, zones ascending.  Events beyond max_events are not stored: status bit 2; event_count and the counters still count them.
 *
 * Outputs: inside int32 [L, M] (bit z: the anchor is in zone z; 0 for a row that is not present); dwell int32 [L, M, Z]; occupancy int32
 * [L, Z]; zone_counts int64 [L, Z, 2] cumulative (enters, exits) and line_counts int64 [L, Ln, 2] cumulative (forward, backward) of the
 * stream; events int64 [L, max_events, 4], zero rows behind the stored ones; event_count int32 [L], the true number.
 * status int32 [S, 2], sticky (the caller clears it): word 0 the bits above, word 1 the `step` of the first event.
 *
 * State: cnl_track_zones_state_bytes(S, max_tracks, Z, Ln) bytes (0 for sizes outside the limits), zeroed by the caller, 8-byte aligned: two
 * banks [2][S] of one stream's block { int64 zone_counts[Z][2], line_counts[Ln][2]; int32 n_entries, 0; int64 id[E]; double anchor[E][2];
 * int32 inside[E], age[E], dwell[E][Z] }.  A call reads bank `bank` and writes the other one — a stream that takes no part is copied —, so the
 * caller alternates `bank`.  Zeroing a stream's block of the current bank forgets the stream.
 * One workgroup per slot; no float atomics, integer LDS adds of ballot popcounts: the same bits on every run.
 * CNL_E_BAD_ARG before any HIP call: a null struct or pointer (dwell / occupancy / zone_counts may be null with Z = 0, line_counts with Ln =
 * 0), S outside 1 .. 65535, L outside 1 .. S, max_tracks outside 1 .. 4096, M outside 1 .. max_tracks, Z or Ln outside 0 .. 16, max_events
 * outside 1 .. 65536, max_absent < 0, anchor / boxes_f64 / bank not 0 or 1, a misaligned pointer (8 bytes: int64 / float64 arrays, geometry,
 * state; 4 bytes: the others).
 */
typedef struct cnl_track_zones {       /* 168 bytes */
    const void* boxes;
    const int64_t* track_ids;
    const int64_t* labels;
    const int32_t* count;
    const int32_t* live;
    const void* geometry;
    void* state;
    int32_t* status;
    int32_t* inside;
    int32_t* dwell;
    int32_t* occupancy;
    int64_t* zone_counts;
    int64_t* line_counts;
    int64_t* events;
    int32_t* event_count;
    int32_t S, L, M, max_tracks;
    int32_t Z, Ln, max_events, max_absent;
    int32_t anchor, boxes_f64, bank, step;
} cnl_track_zones;
int64_t cnl_track_zones_state_bytes(int32_t S, int32_t max_tracks, int32_t Z, int32_t Ln);
int cnl_track_zones_f64(const cnl_track_zones* p, void* stream);

/*
 * Wire formats: COCO boxes are xywh — torchvision box_convert(boxes, "xyxy", "xywh") of
 * CenterNet.validation_step (models/centernet.py:207): out[i] = (x1, y1, x2 - x1, y2 - y1); n boxes of 4 floats, may be in place.
 * boxes and out are 16-byte aligned (a box is moved as one 16-byte word; CNL_E_BAD_ARG otherwise).
 */
int cnl_boxes_xyxy_to_xywh_f32(const float* boxes, float* out, int64_t n, void* stream);

/*
 * The validation value of the detection losses (reference models/centernet.py:123-200 compute_loss / update_heatmap, losses/heatmap_losses.py,
 * losses/box_losses.py; csrc/det_loss.hip): Gaussian target heatmap, heatmap loss and the 3x3 centre-sampled box loss of a batch in one call.
 * This entry point is the value (validation curves, checkpoint selection, regression checks of converted weights); its gradient with respect to the
 * logits and the box values is cnl_detection_loss_grad_f32 below; the tracking model's third loss, the re-ID loss, is cnl_reid_loss_f64 further down.  Every step the
 * reference does on the host in float64 is float64 here; det_loss.hip is compiled with contraction off.  tests/loss_ref.py restates the rule in numpy.
 *
 * Targets: gt_boxes [N, Gmax, 4] float64 x y w h in INPUT pixels, gt_labels [N, Gmax] int64, gt_count [N] int32 (clamped to 0..Gmax), Gmax <= 1024.
 * Slots at or beyond gt_count[n] are never read.
 * Record of a box, float64:  b = box / stride;  cx = rint(b.x + b.w / 2), cy likewise (ties to even: numpy's round);
 *   radius by target_method:  0 "cornernet": the three quadratics of centernet.py:38-58 with min_overlap = target_param (0 < . < 1), r = min(r1, r2, r3),
 *   rx = ry = r;  1 "ttfnet": rx = b.w / 2 * target_param, ry = b.h / 2 * target_param;  2 "fixed": rx = ry = target_param;
 *   then rx = max(0, rint(rx)), ry likewise;  sx = rx / 3 + 1 / 6, sy likewise.
 * A box is SKIPPED whole (nothing rendered, nothing counted, no samples; it adds one to skipped[0]) when one of its numbers or radii is not finite, when
 * w < 0 or h < 0, when its centre lies outside 0 <= cx <= W, 0 <= cy <= H, or when its label lies outside 0 .. C-1.
 * Target value of class `label` at (x, y), 0 <= x < W, 0 <= y < H, |x - cx| <= rx, |y - cy| <= ry (a centre ON cx == W or cy == H has no peak inside the
 * map but renders the part of its window that is inside, as the reference's slices do; it is counted and has its samples):
 *   g = fl32(fl32(dx dx) / fl32(2 sx sx)) + fl32(fl32(dy dy) / fl32(2 sy sy)) added in fp32;  t = fl32(exp(-(double)g));  t = 0 where t < FLT_EPSILON;
 * the target of an element is the maximum over the image's boxes of that class, 0 where no window reaches it; a peak inside the map is exactly 1.0f.
 * Heatmap loss per element, float64, x the fp32 logit and t the fp32 target widened; p = 1 / (1 + exp(-x)), logsigmoid(x) = min(x, 0) - log1p(exp(-|x|)):
 *   heatmap_loss 0 "cornernet_focal":  -(1 - p)^hm_alpha logsigmoid(x) [t == 1]  -  p^hm_alpha logsigmoid(-x) (1 - t)^hm_beta     (defaults 2, 4)
 *   heatmap_loss 1 "quality":          |t - p|^hm_beta (max(x, 0) - x t + log1p(exp(-|x|)))                                         (default 2)
 * (exponents 2 and 4 are formed by multiplication).
 * Box loss: every counted box has the samples {cx-1, cx, cx+1} within [0, W-1] x {cy-1, cy, cy+1} within [0, H-1], cx outer.  At a sample the four
 * box_2d values are decoded by the decode's own fp32 rule (cnl_decode_f32 with normalize_boxes = 0: box_log, box_multiplier, clamp at 0, cx + 0.5,
 * times stride — the same device function); the target is (fl32(x), fl32(y), fl32(x + w), fl32(y + h)), the sums formed in float64.  The loss per
 * sample is float64 on those fp32 values: box_loss 0 "l1", 1 "smooth_l1" (beta 1), 2 "iou", 3 "giou", 4 "diou", 5 "ciou", as losses/box_losses.py
 * with eps = 1e-8, summed.
 * Results: per_image [N, 4] float64 rows (heatmap_sum, box_sum, num_dets, num_boxes);  totals [3] float64:
 *   heatmap = sum(heatmap_sum) / max(1, sum(num_dets)),  box_2d = sum(box_sum) / max(1, sum(num_boxes)),  total = heatmap heatmap_weight + box_2d box_weight;
 * skipped [1] int32.  Every summation order is fixed (within a workgroup, over the workgroups of an image, over the images in index order; no
 * floating-point atomics): a result is the same bits on every run, and an image's row does not depend on which other images share the launch.
 * (The order within an image follows the layout path the heatmap's strides select: channel stride 1, W stride 1, or neither.)
 *
 * heat [N, C, H, W] logits and box [N, 4, H, W], fp32, each with the element strides of its logical axes (n, c, y, x), as the decode takes them.
 * Both NULL with a target map: the targets are rendered and counted, the sums are 0.  target_map: NULL (never written), or fp32 [N, C, H, W] with its own
 * strides: every element receives its target.  The workspace holds at least cnl_detection_loss_workspace_bytes(N, Gmax, H, W) bytes and is 16-byte
 * aligned; float64 / int64 arrays are 8-byte aligned.  Four launches on `stream`, no synchronisation, no allocation.  N <= 2^16, C <= 2^16,
 * H, W <= 2^15 (the workspace size is 0 outside these limits).  The struct's size is cnl_sizeof_params(4).
 */
typedef struct cnl_loss_params {
    double stride;             /* output stride of the maps (boxes are divided by it) */
    double target_param;       /* min_overlap / alpha / r of the target method */
    double hm_alpha, hm_beta;  /* exponents of the heatmap loss (quality reads hm_beta only) */
    double heatmap_weight, box_weight;
    float box_multiplier;
    int32_t target_method;     /* 0 cornernet, 1 ttfnet, 2 fixed */
    int32_t heatmap_loss;      /* 0 cornernet_focal, 1 quality */
    int32_t box_loss;          /* 0 l1, 1 smooth_l1, 2 iou, 3 giou, 4 diou, 5 ciou */
    int32_t box_log;
    int32_t reserved;          /* 0 */
} cnl_loss_params;
size_t cnl_detection_loss_workspace_bytes(int32_t N, int32_t Gmax, int32_t H, int32_t W);
int cnl_detection_loss_f64(const float* heat, int64_t heat_sn, int64_t heat_sc, int64_t heat_sh, int64_t heat_sw, const float* box, int64_t box_sn,
                           int64_t box_sc, int64_t box_sh, int64_t box_sw, int32_t N, int32_t C, int32_t H, int32_t W, const double* gt_boxes,
                           const int64_t* gt_labels, const int32_t* gt_count, int32_t Gmax, const cnl_loss_params* p, float* target_map, int64_t t_sn,
                           int64_t t_sc, int64_t t_sh, int64_t t_sw, double* per_image, double* totals, int32_t* skipped, void* workspace,
                           size_t workspace_bytes, void* stream);

/*
 * The gradient of exactly the function cnl_detection_loss_f64 computes, for a criterion training can call (csrc/det_loss.hip; tests/loss_grad_ref.py
 * restates it in numpy): grad_heat = d(s_heat heatmap + s_box box_2d) / d heat, grad_box likewise / d box, where
 *   heatmap = sum of element terms / max(1, num_dets),   box_2d = sum of sample terms / max(1, num_boxes),
 * num_dets and num_boxes counted over the BATCH, the target map a constant and the [t == 1] weight a constant.  Everything is float64 on the fp32
 * logits and the fp32 decoded boxes, rounded ONCE to fp32.
 * Heatmap, every element:  grad_heat[n,c,y,x] = fl32(s_heat / max(1, num_dets) * dterm/dx), with p, ls(x) = logsigmoid(x) and log1p(exp(-|x|)) formed as
 * the forward forms them (dp/dx = p (1 - p), d ls(x)/dx = 1 - p, d ls(-x)/dx = -p), exponents 2 and 4 by multiplication:
 *   "cornernet_focal" (alpha 2):  [t == 1] (1 - p)^2 (2 p ls(x) - (1 - p))  +  (1 - t)^hm_beta p^2 (p - 2 (1 - p) ls(-x))
 *       (any alpha: [t == 1] (alpha (1-p)^(alpha-1) p (1-p) ls(x) - (1-p)^alpha (1-p))  +  (1-t)^hm_beta (p^alpha p - alpha p^(alpha-1) p (1-p) ls(-x)))
 *   "quality" (beta 2):           (t - p)^2 (p - t)  -  sign(t - p) 2 |t - p| p (1 - p) ce,   ce = max(x, 0) - x t + log1p(exp(-|x|))
 *       (any beta: |t-p|^beta (p - t) - sign(t-p) beta |t-p|^(beta-1) p (1-p) ce);  exactly 0 at t == p.
 * Box: for every counted box and each of its up to nine samples, the derivative of the sample's loss with respect to the four box values at that pixel:
 * through the loss (l1, smooth_l1, iou, giou, diou, ciou on the fp32 decoded box and the fp32 target, eps 1e-8; ciou's alpha is differentiated, as the
 * reference's autograd does) and through the decode: d x1 / d v = -stride box_multiplier [fl32(v' box_multiplier) >= 0] (exp(v) with box_log, as the
 * decode's fp32 expf gives it; v' = that exp or v), + for x2, y2.  A pixel sampled by several boxes receives the SUM of their contributions, added in
 * float64 in slot order (a box samples a pixel at most once):  grad_box[n,j,y,x] = fl32(s_box / max(1, num_boxes) * sum);  a pixel no sample touches
 * receives exactly 0.
 * Non-differentiable points follow torch's autograd: the clamps at 0 (decode, intersection) pass the gradient where the clamped value is >= 0;
 * maximum / minimum give half to each side on a tie;  |d| has derivative 0 at 0;  smooth_l1 takes the quadratic branch for |d| < 1;
 * |t - p|^beta has derivative 0 at t == p.  A skipped box contributes nothing and is counted in skipped[0], as in the forward.
 *
 * heat, box, the targets, p and the limits: as cnl_detection_loss_f64 (heat and box both non-NULL).  scales: DEVICE float64 [2] = (s_heat, s_box), read by
 * the kernels (no synchronisation for a caller whose scales are computed on the device); NULL: 1, 1.  grad_heat [N, C, H, W] and grad_box [N, 4, H, W],
 * fp32, each with its own element strides; NULL: not wanted (its launch is skipped).  Every element of a wanted output is written exactly once: no
 * pre-zeroing, and nothing outside the declared elements or past workspace_bytes is written.  The element order of the heatmap gradient follows
 * grad_heat's strides (channel stride 1, W stride 1, or neither); where heat and grad_heat are both packed channels-last (pixel stride C, the other
 * strides and W C multiples of 4, bases 16-byte aligned) a lane moves four consecutive elements per 16-byte access.  The workspace holds at least
 * cnl_detection_loss_grad_workspace_bytes(N, Gmax, H, W) bytes (0 outside the limits), 16-byte aligned.  At most four launches on `stream` (records,
 * counts, heatmap gradient, box gradient), no synchronisation, no allocation, no memset, no atomics: the same bits on every run.
 */
size_t cnl_detection_loss_grad_workspace_bytes(int32_t N, int32_t Gmax, int32_t H, int32_t W);
int cnl_detection_loss_grad_f32(const float* heat, int64_t heat_sn, int64_t heat_sc, int64_t heat_sh, int64_t heat_sw, const float* box, int64_t box_sn,
                                int64_t box_sc, int64_t box_sh, int64_t box_sw, int32_t N, int32_t C, int32_t H, int32_t W, const double* gt_boxes,
                                const int64_t* gt_labels, const int32_t* gt_count, int32_t Gmax, const cnl_loss_params* p, const double* scales,
                                float* grad_heat, int64_t gh_sn, int64_t gh_sc, int64_t gh_sh, int64_t gh_sw, float* grad_box, int64_t gb_sn,
                                int64_t gb_sc, int64_t gb_sh, int64_t gb_sw, int32_t* skipped, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The re-ID loss of the tracking model (reference models/fairmot.py:34-61 EmbeddingHead.compute_loss; csrc/reid_loss.hip; tests/reid_loss_ref.py restates
 * the rule in numpy): the embedding at every box centre goes through the training-only classifier Linear(D, D, no bias) / BatchNorm1d(D) / ReLU /
 * Linear(D, K) and a cross entropy over the K track identities.  Value and analytic gradient, float64 on the fp32 values, every summation order fixed:
 * no atomics, no memset, the same bits on every run.  The R x K logits (R = N Gmax) are never written to memory.
 *
 * Inputs: reid [N, D, H, W] fp32 with the element strides of its logical axes (n, c, y, x); gt_boxes [N, Gmax, 4] float64 x y w h in INPUT pixels,
 * gt_ids [N, Gmax] int64, gt_count [N] int32 (clamped to 0..Gmax); the classifier, fp32, dense: W1 [D, D], gamma / beta / running_mean / running_var [D],
 * W2 [K, D], b2 [K].
 * Rows: row r = (n, g), taken in (n, g) order.  A LIVE row has g < gt_count[n], finite box numbers, w >= 0, h >= 0, 0 <= id < K, and its cell inside the
 * map: c = (b.x + b.w / 2) / stride, x = trunc(c) (center 0, the reference's .long()) or rint(c) (center 1: the peak cell of the detection loss's record
 * rule), y likewise, 0 <= x <= W - 1, 0 <= y <= H - 1.  A row with g < gt_count[n] and id == ignore_index is dropped silently; any other row with
 * g < gt_count[n] that is not live is skipped and counted.  STAT rows (those the BatchNorm statistics are taken over): the live rows, and with
 * padded_rows = 1 also every slot g >= gt_count[n], which reads cell (0, 0) of its image and enters the statistics but not the loss (what the
 * reference's zero-padded boxes and mask do).  R_s stat rows, M live rows.
 * Forward, float64:  e_r = the D values at the cell;  h_j = sum_i W1[j, i] e_i by fused multiply-add, i ascending;
 *   training = 1: mean_j = (sum over the stat rows, ascending r, of h_j) / R_s, var_j = (sum, ascending r, of (h_j - mean_j)^2) / R_s;
 *     new_stats = fl32((1 - momentum) running + momentum (mean, var R_s / (R_s - 1)));   training = 0: mean, var = the running statistics;
 *   a_j = (h_j - mean_j) / sqrt(var_j + bn_eps) * gamma_j + beta_j;  z_j = max(a_j, 0);
 *   logit_k = b2_k, then fma(z_j, W2[k, j], logit_k) for j ascending;
 *   log-sum-exp over tiles of 64 identities, tiles ascending, with a running (m, s): in a tile t = its maximum, m' = max(m, t); 16 partial sums, partial q
 *     = exp(logit - m') of identities 4q .. 4q + 3 of the tile added in ascending order (0 beyond K); the 16 partials folded by a butterfly (partners at
 *     distance 1, 2, 4, 8); s = s exp(m - m') + that sum, m = m';  lse_r = m + log(s);  ce_r = lse_r - logit_id;  top-1: the first of the largest logits;
 *   total = (sum of ce_r over the live rows, ascending r) / (M + 1e-8).
 * training = 1 with R_s < 2: total 0, per_row 0, every gradient 0, new_stats = the running statistics, counts[3] = 0 (torch raises there; a batch without
 * identities must not stop a run).
 * Results of cnl_reid_loss_f64: per_row [N, Gmax] float64 (ce_r, 0 for rows not in the loss; every element written), total [1] float64, counts [4] int32 =
 * (M, top-1 hits, skipped rows, 1 when the running statistics made a step), new_stats [2, D] fp32 (NULL: not wanted).  The running statistics themselves
 * are never written.
 *
 * cnl_reid_loss_grad_f32: d(scale total) / d(reid, W1, gamma, beta, W2, b2), float64 rounded ONCE to fp32.  scale: DEVICE float64 [1], read by the
 * kernels; NULL: 1.  With p_k = exp(logit_k - lse_r):  g[r, k] = scale (p_k - [k == id_r]) / (M + 1e-8) on live rows;
 *   grad_W2[k, j] = sum over the live rows, ascending r, of g[r, k] z[r, j];  grad_b2[k] = that sum of g[r, k];  dz[r, j] = sum_k g[r, k] W2[k, j], k ascending;
 *   da = dz where z > 0, else 0 (the ReLU's derivative is 0 at a <= 0);  grad_beta_j = sum da, grad_gamma_j = sum da xhat (live rows, ascending r),
 *   xhat = (h - mean) / sqrt(var + bn_eps);  dxhat = da gamma;
 *   training = 1: dh = (R_s dxhat - sum dxhat - xhat sum(dxhat xhat)) / (R_s sqrt(var + bn_eps)) on EVERY stat row (a padded row has dxhat = 0 but
 *   receives a gradient through the batch statistics);  training = 0: dh = dxhat / sqrt(var + bn_eps);
 *   grad_W1[j, i] = sum over the stat rows, ascending r, of dh[r, j] e[r, i];  de[r, i] = sum_j W1[j, i] dh[r, j], j ascending;
 *   grad_reid [N, D, H, W] with its own strides: a cell receives the sum of its stat rows' de in (n, g) order (several boxes can share a cell, padded rows
 *   all share (0, 0)); every other element is exactly 0; every element is stored exactly once by the workgroup that owns its 8 x 32 pixel tile.
 * Any gradient pointer may be NULL (not wanted; its launches are skipped).  skipped [1] int32 (NULL: not wanted).
 *
 * Limits (CNL_E_BAD_ARG outside them): 1 <= D <= 256, 2 <= K <= 2^20, Gmax <= 1024, N <= 2^16, H, W <= 2^15.  The workspace holds at least
 * cnl_reid_loss_workspace_bytes / cnl_reid_loss_grad_workspace_bytes (N, Gmax, D) bytes (0 outside the limits) and is 16-byte aligned; float64 / int64
 * arrays are 8-byte aligned.  Launches on `stream` only, no synchronisation, no allocation.  The struct's size is cnl_sizeof_params(5).
 */
typedef struct cnl_reid_loss_params {
    double stride;             /* output stride of the map (box centres are divided by it) */
    double bn_eps;             /* BatchNorm1d.eps */
    double momentum;           /* BatchNorm1d.momentum (a number) */
    int64_t ignore_index;      /* identity of a box without one: the row is dropped silently */
    int32_t center;            /* 0 trunc, 1 round */
    int32_t padded_rows;       /* 1: slots beyond gt_count are stat rows at cell (0, 0) */
    int32_t training;          /* 1: batch statistics; 0: running statistics */
    int32_t reserved;          /* 0 */
} cnl_reid_loss_params;
size_t cnl_reid_loss_workspace_bytes(int32_t N, int32_t Gmax, int32_t D);
int cnl_reid_loss_f64(const float* reid, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int32_t N, int32_t D, int32_t H, int32_t W, const double* gt_boxes,
                      const int64_t* gt_ids, const int32_t* gt_count, int32_t Gmax, const float* W1, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, const float* W2, const float* b2, int32_t K, const cnl_reid_loss_params* p,
                      double* per_row, double* total, int32_t* counts, float* new_stats, void* workspace, size_t workspace_bytes, void* stream);
size_t cnl_reid_loss_grad_workspace_bytes(int32_t N, int32_t Gmax, int32_t D);
int cnl_reid_loss_grad_f32(const float* reid, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int32_t N, int32_t D, int32_t H, int32_t W,
                           const double* gt_boxes, const int64_t* gt_ids, const int32_t* gt_count, int32_t Gmax, const float* W1, const float* gamma,
                           const float* beta, const float* running_mean, const float* running_var, const float* W2, const float* b2, int32_t K,
                           const cnl_reid_loss_params* p, const double* scale, float* grad_reid, int64_t gn, int64_t gc, int64_t gh, int64_t gw,
                           float* grad_W1, float* grad_gamma, float* grad_beta, float* grad_W2, float* grad_b2, int32_t* skipped, void* workspace,
                           size_t workspace_bytes, void* stream);

/*
 * Training augmentation of a batch: the reference's albumentations Compose (HorizontalFlip, RandomResizedCrop, ColorJitter, Cutout:
 * datasets/builder.py::parse_transforms, one image at a time on the host) and a batch-level mosaic (datasets/transforms.py declares
 * Mosaic.__call__ with an empty body) as TWO launches that are a deterministic function of a PLAN.  All randomness is drawn on the host into
 * the plan; nothing below is random, nothing goes to the host, no atomics: the same plan gives the same bytes on every run.
 *
 * The plan of N canvases of height x width (new entry points and records only: the ABI version does not change):
 *   places   device array of N * 4 placement records (four slots per canvas), 96 bytes each, 8-byte aligned:
 *     offset  0  int32 frame            index of the source frame, 0..F-1
 *     offset  4  int32 x0, y0, w, h     the source window inside that frame: w, h >= 1, x0, y0 >= 0, x0 + w <= frame w, y0 + h <= frame h
 *     offset 20  int32 dx0, dy0, dw, dh the destination rectangle inside the canvas: dx0 % 4 == 0, dw % 4 == 0, dw >= 4, dh >= 1
 *     offset 36  int32 flip             != 0: mirrored left-right inside the rectangle
 *     offset 40  int32 colour[12]       Q12 colour matrix: colour[3c + k] (|.| <= 32767) weighs source channel k in channel c; colour[9 + c]
 *                                       (|.| <= 2^21) is channel c's offset, already multiplied by 4096.  Identity: 4096 at 0, 4, 8, else 0.
 *     offset 88  int32 reserved[2]      0
 *   n_place  N int32 in device memory: the live slots of canvas n are 0 .. n_place[n] - 1.  The kernels clamp it to 0..max_place, and
 *            max_place (1..4, a host argument: the largest n_place of the plan) is what the host can check.
 *   holes    N * 16 slots of four int32 (x0, y0, w, h) in canvas pixels, 16-byte aligned, or NULL for no holes; w <= 0 or h <= 0 marks a dead
 *            slot.  Holes may overlap each other and the canvas edge (x0, y0 may be negative); they are clipped to the canvas.
 * The rectangles of one canvas should be disjoint; where two overlap, the lower slot wins.  A DEGENERATE record — frame outside 0..F-1, a
 * window that is empty or leaves its frame, a rectangle that is empty, misaligned or leaves the canvas — is not a fault: it paints nothing
 * (cnl_augment_u8) and carries no boxes (cnl_augment_boxes_f64, which cannot see frame sizes and judges frame, w, h, dw, dh only).
 *
 * cnl_augment_u8.  frames: device array of F WHOLE-FRAME cnl_letterbox_frame records of 3-channel packed frames (only src, h, w and
 * row_stride are read).  out: [N, height, width, 3] u8, 4-byte aligned, height in 1..32768, width in 4..32768 a multiple of 4; every byte is
 * written exactly once in one launch (no memset before it).  The value of canvas pixel (y, x), byte c = bits 8c..8c+7 of a word:
 *   inside the rectangle of placement p, at dy = y - dy0, dx = x - dx0: the cv2 INTER_LINEAR resize of the window (h, w) -> (dh, dw) at
 *     (dy, dx') with dx' = flip ? dw - 1 - dx : dx, in exactly the arithmetic of cnl_letterbox_bilinear_u8 (cnl_resize_bilinear_u8's 8-bit
 *     fixed-point rule, the taps clipped to the window as cnl_crop_boxes_u8 clips them), giving R, G, B; then for c in 0..2, in 32-bit integers,
 *     >> an arithmetic shift (floor):
 *         out_c = clamp((colour[3c] * R + colour[3c + 1] * G + colour[3c + 2] * B + colour[9 + c] + 2048) >> 12, 0, 255)
 *   in no rectangle: fill_rgba
 *   in a hole: hole_fill_rgba, overriding both.
 * A placement with flip = 0, the identity matrix and no hole is therefore bit for bit what cnl_letterbox_bilinear_u8 writes for the record
 * (h, w, new_h = dh, new_w = dw, pad_top = dy0, pad_left = dx0) on the sliced frame.  YUV sources are not taken.
 *
 * cnl_augment_boxes_f64.  The targets in the padded forms of cnl_detection_loss_f64: boxes [F, Gmax, 4] f64 (x, y, w, h: top-left corner and
 * size in the SOURCE frame's pixels), labels [F, Gmax] i64, ids [F, Gmax] i64 (optional, given together with out_ids), count [F] i32 (clamped
 * to 0..Gmax).  Outputs: out_boxes [N, Gout, 4] f64 in CANVAS pixels, out_labels / out_ids [N, Gout] i64, out_count [N] i32, with
 * Gout >= max_place * Gmax.  For canvas n, placements in slot order and, within a placement, boxes j < count[frame] in source order; every step
 * is ONE float64 operation in the order written (no fused multiply-add):
 *     sx = dw / w, sy = dh / h                                  (the int32 values converted to double)
 *     u1 = (x - x0) * sx, u2 = ((x + bw) - x0) * sx;  v1 = (y - y0) * sy, v2 = ((y + bh) - y0) * sy
 *     flip != 0: t = dw - u2, u2 = dw - u1, u1 = t
 *     full = (u2 - u1) * (v2 - v1)
 *     cu1 = min(max(u1, 0), dw), cu2 = min(max(u2, 0), dw), cv1 = min(max(v1, 0), dh), cv2 = min(max(v2, 0), dh)
 *     cw = cu2 - cu1, ch = cv2 - cv1, area = cw * ch
 * The box is KEPT iff x, y, bw, bh, u1, u2, v1, v2 and full are all finite, cw > 0, ch > 0, area >= min_area (albumentations'
 * BboxParams(min_area); the reference uses 1), area >= min_visibility * full, and its label is >= 0.  A kept box is written as
 * (dx0 + cu1, dy0 + cv1, cw, ch) with its label and id.  Kept boxes are compacted STABLY (slot order, then source order) into slots
 * 0 .. out_count[n] - 1; every slot beyond is exactly zero (boxes, labels, ids).  Holes do not touch boxes (as in albumentations).
 *
 * Both: N, F in 0..65535; N == 0 is a no-op.  CNL_E_BAD_ARG with a message for everything the host can see, before anything is launched.
 */
typedef struct cnl_augment_placement {
    int32_t frame;
    int32_t x0, y0, w, h;
    int32_t dx0, dy0, dw, dh;
    int32_t flip;
    int32_t colour[12];
    int32_t reserved[2];
} cnl_augment_placement;
int cnl_augment_u8(const void* frames, int32_t F, const void* places, const int32_t* n_place, int32_t max_place, const int32_t* holes, uint8_t* out,
                   int32_t N, int32_t height, int32_t width, uint32_t fill_rgba, uint32_t hole_fill_rgba, void* stream);
int cnl_augment_boxes_f64(const void* places, const int32_t* n_place, int32_t max_place, int32_t N, int32_t F, const double* boxes,
                          const int64_t* labels, const int64_t* ids, const int32_t* count, int32_t Gmax, double* out_boxes, int64_t* out_labels,
                          int64_t* out_ids, int32_t* out_count, int32_t Gout, double min_area, double min_visibility, void* stream);

/*
 * Affine training augmentation: the geometric transforms of the reference's training lists that are not separable — albumentations' Affine
 * (scale, rotate, shear, translate), and with it RandomResizedCrop / RandomCrop / SmallestMaxSize and HorizontalFlip — composed by the host
 * into ONE affine map per placement, so that every canvas pixel is resampled ONCE.  The plan, n_place, max_place, holes, the canvas, the
 * limits, the degenerate-record rule and the no-op N == 0 are those of cnl_augment_u8 / cnl_augment_boxes_f64 above; the record differs
 * (new entry points and a new record only: the ABI version does not change):
 *   places   device array of N * 4 warp records, 192 bytes each, 8-byte aligned:
 *     offset   0  int32  frame
 *     offset   4  int32  x0, y0, w, h      the CLIP window in the source frame (the whole frame: 0, 0, frame w, frame h); bounds as above
 *     offset  20  int32  dx0, dy0, dw, dh  the destination rectangle; bounds as above
 *     offset  36  int32  reserved0         0
 *     offset  40  int32  colour[12]        the Q12 matrix of cnl_augment_placement, same bounds
 *     offset  88  int64  inv[6]            Q20 inverse map: canvas pixel (dx, dy) of the rectangle -> source pixel INDEX
 *     offset 136  double fwd[6]            forward map: continuous source-frame coordinates -> continuous rectangle coordinates
 *     offset 184  int32  reserved[2]       0
 * A mirror is not a field: the host folds it into both maps.  A record is also DEGENERATE (paints nothing, carries no boxes) when
 * |inv[0]|, |inv[1]|, |inv[3]| or |inv[4]| > 2^30 or |inv[2]| or |inv[5]| > 2^44.
 *
 * cnl_augment_warp_u8.  cnl_augment_u8's arguments with warp records and border_rgba, the colour of everything outside the clip window.
 * Inside the rectangle of placement p, at dx = x - dx0, dy = y - dy0, all in exact integers (>> an arithmetic shift: floor):
 *     X  = inv[0]*dx + inv[1]*dy + inv[2]        Y  = inv[3]*dx + inv[4]*dy + inv[5]        (int64)
 *     sx = X >> 20,  sy = Y >> 20
 *     a1 = (X >> 9) & 2047, a0 = 2048 - a1       b1 = (Y >> 9) & 2047, b0 = 2048 - b1
 *     tap(i, j), i, j in {0, 1}: channel c of frame pixel (sx + i, sy + j) if x0 <= sx+i < x0+w and y0 <= sy+j < y0+h, else byte c of border_rgba
 *     t = tap(0,0)*a0 + tap(1,0)*a1              u = tap(0,1)*a0 + tap(1,1)*a1
 *     v = (t*b0 + u*b1 + 2^21) >> 22             (fits int32; 0..255 without a clamp)
 * giving (R, G, B) = v; then cnl_augment_u8's colour step, unchanged — so the border is jittered too, as albumentations' ColorJitter after
 * Affine does.  In no rectangle: fill_rgba; in a hole: hole_fill_rgba; where rectangles overlap the lower slot wins.  Every canvas byte is
 * written exactly once in one launch.  This rule is deliberately NOT cv2.warpAffine's (5-bit weights from a 10-bit table of rounded
 * coordinates) and NOT the letterbox rule (cv2 INTER_LINEAR resize with separable float-derived weights): it is the cheapest exact-integer
 * rule a rotated gather admits.  Consequences: an identity or integer-translation map copies source bytes exactly; quarter turns and mirrors
 * are exact permutations.  No frame byte outside [row start, row start + 3 * frame w) of a frame row is read, and a pixel whose four taps
 * all lie outside the window reads nothing.
 *
 * The host rule warp_inverse(fwd) -> inv, in float64, each operation rounded on its own, in the order written:
 *     det = fwd[0]*fwd[4] - fwd[1]*fwd[3];  A00 = fwd[4]/det, A01 = -fwd[1]/det, A10 = -fwd[3]/det, A11 = fwd[0]/det  (the 2 x 2 adjugate)
 *     A02 = -(A00*fwd[2] + A01*fwd[5]),  A12 = -(A10*fwd[2] + A11*fwd[5])
 *     inv[0,1,3,4] = rint(A_ij * 2^20)
 *     inv[2] = rint((((0.5*A00 + 0.5*A01) + A02) - 0.5) * 2^20),  inv[5] = rint((((0.5*A10 + 0.5*A11) + A12) - 0.5) * 2^20)
 * the pixel-centre convention: pixel k covers [k, k + 1).  A singular or non-finite map, or one outside the bounds above, is refused.
 *
 * cnl_augment_warp_boxes_f64.  cnl_augment_boxes_f64's arguments with warp records.  Every step is ONE float64 operation in the order
 * written (no fused multiply-add):
 *     corners (X, Y) in the order a = (x, y), b = (x+bw, y), c = (x, y+bh), d = (x+bw, y+bh)
 *     u_k = (fwd[0]*X + fwd[1]*Y) + fwd[2],   v_k = (fwd[3]*X + fwd[4]*Y) + fwd[5]
 *     u1 = min(min(min(u_a, u_b), u_c), u_d), u2 = the same with max;  v1, v2 likewise
 * the enclosing box (albumentations' rotate_method="largest_box"); from full = (u2 - u1)*(v2 - v1) on it is cnl_augment_boxes_f64's rule
 * exactly (clip to [0, dw] x [0, dh]; KEPT iff x, y, bw, bh, every u_k and v_k and full are finite, cw > 0, ch > 0, area >= min_area,
 * area >= min_visibility * full, label >= 0; written as (dx0 + cu1, dy0 + cv1, cw, ch); compacted STABLY; every slot beyond is zero).  This
 * entry judges a record by frame, w, h, dw, dh and the bounds of inv.
 */
typedef struct cnl_warp_placement {
    int32_t frame;
    int32_t x0, y0, w, h;
    int32_t dx0, dy0, dw, dh;
    int32_t reserved0;
    int32_t colour[12];
    int64_t inv[6];
    double fwd[6];
    int32_t reserved[2];
} cnl_warp_placement;
int cnl_augment_warp_u8(const void* frames, int32_t F, const void* places, const int32_t* n_place, int32_t max_place, const int32_t* holes,
                        uint8_t* out, int32_t N, int32_t height, int32_t width, uint32_t fill_rgba, uint32_t hole_fill_rgba, uint32_t border_rgba,
                        void* stream);
int cnl_augment_warp_boxes_f64(const void* places, const int32_t* n_place, int32_t max_place, int32_t N, int32_t F, const double* boxes,
                               const int64_t* labels, const int64_t* ids, const int32_t* count, int32_t Gmax, double* out_boxes, int64_t* out_labels,
                               int64_t* out_ids, int32_t* out_count, int32_t Gout, double min_area, double min_visibility, void* stream);

/*
 * Pixel-level training augmentation: the transforms of the reference's training lists that need a neighbourhood or a histogram — MotionBlur
 * (configs/crowdhuman_tracking.yaml) and the photometric members of datasets/transforms.py::TrivialAugmentWide (Sharpen, Posterize, Solarize,
 * Equalize).  A FINISHED canvas batch [N, height, width, 3] u8 (what cnl_augment_u8 / cnl_augment_warp_u8 wrote) goes through ONE operation
 * per canvas, then that canvas's holes are punched (the reference's order: Cutout last, so a hole's edge is sharp and its colour does not
 * bleed).  Everything is integer arithmetic; nothing is random, nothing goes to the host, no global atomics: the same bytes on every run, and
 * a canvas's bytes do not depend on its batch.  New entry points and a new record only: the ABI version does not change.
 *
 *   ops      device array of N records, 400 bytes each, 4-byte aligned:
 *     offset   0  int32 op             CNL_PIXEL_NONE / FILTER / POSTERIZE / SOLARIZE / EQUALIZE
 *     offset   4  int32 param          POSTERIZE: bits, 0..8; SOLARIZE: the threshold t, 0..255; else 0
 *     offset   8  int32 n_taps         FILTER: 1..32; else 0
 *     offset  12  int32 reserved       0
 *     offset  16  int32 taps[32][3]    FILTER: (dx, dy, w) with |dx|, |dy| <= 15, w signed; sum w = 65536 exactly, sum |w| <= 2^23
 *   holes    cnl_augment_u8's: N * 16 slots (x0, y0, w, h), 16-byte aligned, or NULL; punched with hole_fill_rgba AFTER the operation
 *   launches what the host-visible plan holds: 0, CNL_PIXEL_HAS_TABLE (some canvas has POSTERIZE, SOLARIZE or EQUALIZE: the table launch) or
 *            CNL_PIXEL_HAS_TABLE | CNL_PIXEL_HAS_EQUALIZE (also the histogram launch).  Two or three launches, or one.
 *
 * The value of out pixel (y, x), channel c, from the canvas `in` of the same n (>> an arithmetic shift: floor):
 *   NONE       in
 *   FILTER     clamp((sum_i w_i * in[r(y + dy_i, height), r(x + dx_i, width), c] + 32768) >> 16, 0, 255), with r cv2's BORDER_REFLECT_101 made
 *              total: r(i, 1) = 0; otherwise m = i mod 2(n - 1) (non-negative) and r = m if m < n, else 2(n - 1) - m — for a canvas smaller than
 *              the radius too (numpy.pad(mode="reflect")).  A constant canvas is a fixed point of every such filter.
 *   POSTERIZE  v & (0xFF << (8 - bits)) & 0xFF          SOLARIZE  v >= t ? 255 - v : v          (albumentations' tables)
 *   EQUALIZE   albumentations' default (mode="cv", by_channels), per channel: h the channel's histogram over the whole canvas (before the
 *              holes), i0 its first populated bin, d = height * width - h[i0]; d == 0 leaves the channel unchanged; otherwise lut[v] = 0 for
 *              v <= i0 and lut[v] = (510 * cum(v) + d) / (2 d) (floor, 64-bit) with cum(v) = sum_{i0 < i <= v} h[i].  DEVIATION: cv2.equalizeHist
 *              rounds cum * (255.f / d) in fp32, which differs from this exact rounding in a few table entries, by one level.
 *   in a hole  hole_fill_rgba, overriding all of them.
 * The MotionBlur and Sharpen taps are the host's (centernet_lightning_amd/pixel.py: the line rule and a = rint(alpha * 65536)).
 *
 * A BAD record is not a fault and can never index out of the kernel's LDS: a record whose op is none of the five, a FILTER with n_taps
 * outside 1..32, any |dx| or |dy| > 15 or sum |w| > 2^23, and a POSTERIZE / SOLARIZE whose param is out of range all run as NONE (the canvas
 * is copied and its holes punched: skipped, not clamped).  The sum of the weights is the host's to check; the device does not.  A table
 * operation in a call whose `launches` lacks CNL_PIXEL_HAS_TABLE runs as NONE, and an EQUALIZE without CNL_PIXEL_HAS_EQUALIZE gets the identity
 * table: a wrong `launches` never reads workspace bytes that were not written.
 *
 * workspace: exactly cnl_augment_pixel_workspace_bytes(N, height, width) bytes (a pure host function, monotone in each argument; 0 for
 * arguments the entry refuses and for N == 0), 16-byte aligned: N * 768 table bytes, then N * min(ceil(height / 8), 32) partial histograms of
 * 768 uint32.  It need not be cleared.  canvas is only read; out [N, height, width, 3] u8 must not overlap it (refused) and every byte of it is
 * written exactly once.  canvas, out: 4-byte aligned; height in 1..32768, width in 4..32768 a multiple of 4; N in 0..65535, N == 0 a no-op.
 * CNL_E_BAD_ARG (CNL_E_WORKSPACE for the size) with a message for everything the host can see, before anything is launched.
 */
#define CNL_PIXEL_NONE 0
#define CNL_PIXEL_FILTER 1
#define CNL_PIXEL_POSTERIZE 2
#define CNL_PIXEL_SOLARIZE 3
#define CNL_PIXEL_EQUALIZE 4
#define CNL_PIXEL_MAX_TAPS 32
#define CNL_PIXEL_MAX_RADIUS 15
#define CNL_PIXEL_HAS_TABLE 1
#define CNL_PIXEL_HAS_EQUALIZE 2
typedef struct cnl_pixel_op {
    int32_t op;
    int32_t param;
    int32_t n_taps;
    int32_t reserved;
    int32_t taps[CNL_PIXEL_MAX_TAPS][3];
} cnl_pixel_op;
size_t cnl_augment_pixel_workspace_bytes(int32_t N, int32_t height, int32_t width);
int cnl_augment_pixel_u8(const uint8_t* canvas, int32_t N, int32_t height, int32_t width, const void* ops, int32_t launches, const int32_t* holes,
                         uint32_t hole_fill_rgba, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ---- Convolution gradients: fine-tuning the heads (csrc/conv_grad.hip; no ABI bump: new entry points only) ----
 * The backward pass of  z = conv(x, w) + bias, y = relu(z)  for the stride-1 3x3 / pad 1 and 1x1 / pad 0 convolutions of a head
 * (reference models/meta.py:21-30), given the loss gradient dy.  LAYOUT: every tensor is NHWC fp32 with a pixel stride in elements
 * (ldx >= Cin, lddz >= Cout, lddx >= Cin; each % 4 == 0 and each of x, dz, dx, dw, w and the wgrad workspace 16-byte aligned, else
 * CNL_E_BAD_ARG), so a tensor may be a channel slice of a wider buffer; a tensor spans at most the engine's 4 GiB addressing
 * (N * H * W * ld * 4 <= 0xEF000000, else CNL_E_UNSUPPORTED: split the batch).  OUTPUT CONTRACT, as for the conv family: an entry point
 * writes its declared channels of its declared pixels (dw: all Cout * KH * KW * Cin floats) and nothing else.  DETERMINISM: no atomics and
 * no memset; partial results go to a workspace that need not be cleared and are added in a fixed order — the same bytes on every run.
 * ARITHMETIC: fp32 only.  The weight gradient runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, bit for bit an
 * fmaf chain in pixel order); the 1x1 input gradient is an fmaf chain over co = 0, 1, ... on the vector ALU.  The scaled two-way fp16
 * split of the forward kernels is NOT used: it promises fp32-level results for inputs within 1e4 of the image maximum, and a loss
 * gradient map (the focal loss at a box centre beside far negatives) spans many more decades.  The 3x3 INPUT gradient needs no entry
 * point of its own: dx = conv3x3(dz, w rotated by 180 degrees with O and I swapped) is cnl_conv2d_nhwc_f32 without x_absmax / w_absmax
 * (Cin of that call = Cout of the layer, so Cout % 32 == 0).  Every refusal happens before anything is launched, with cnl_last_error text.
 *
 * cnl_relu_grad_f32: dz[p][c] = y[p][c] > 0 ? dy[n][c][h][w] : 0 (torch's ReLU backward: exactly 0 where y == 0; a NaN y gives 0), for
 *   p = (n * H + h) * W + w; y == NULL: a plain copy into the dz layout (a conv without activation).  dy: element strides of the logical
 *   axes (n, c, h, w), any non-negative values, 4-byte aligned; y: [N * H * W][ldy], ldy >= C.  dbias (NULL: not wanted; then no workspace):
 *   dbias[c] = sum_p dz[p][c] — a workgroup owns 256 consecutive pixels and adds them in fp32 (cpt = min(256, C rounded up to a power of
 *   two) threads per pixel, 256 / cpt pixel lanes with stride 256 / cpt, each in pixel order, then the lanes in lane order), the
 *   workgroups' sums are added in workgroup order in float64 and rounded once.  cnl_relu_grad_terms: an upper bound on the roundings on
 *   the path to a dbias element (257).  workspace: cnl_relu_grad_workspace_bytes = ceil(N * H * W / 256) * C * 4 bytes, 4-byte aligned.
 *
 * cnl_conv_wgrad_nhwc_f32: dw[co][ky][kx][ci] = sum over n, oy, ox of dz[n, oy, ox, co] * x[n, oy + ky - pad, ox + kx - pad, ci], zero outside
 *   the image; dw is OHWI and dense, the layout of cnl_conv_params.w.  (KH, KW, pad) = (3, 3, 1) or (1, 1, 0), Cin % 32 == 0 (else
 *   CNL_E_UNSUPPORTED), any Cout >= 1.  A GEMM with M = Cout, N = KH * KW * Cin, K = N * H * W: a workgroup owns 128 couts x all taps x 32
 *   input channels for ONE slice of the image rows (row r = n * H + oy), stages dz and the x rows with their one-pixel halo through LDS
 *   (each x element staged serves all taps), accumulates in pixel order and writes its partial tile to workspace[slice][co][tap][ci]; a
 *   second launch adds the slices in slice order.  THE SLICE FUNCTION (of the layer shape and N, H, W alone — so the result is a function
 *   of the inputs alone): tiles = ceil(Cout / 128) * (Cin / 32); rows = N * H; rows_per_slice = min(rows, max(ceil(rows / ceil(1024 /
 *   tiles)), ceil(512 / W))); slices = ceil(rows / rows_per_slice) = cnl_conv_wgrad_slices (0 for a shape the entry refuses).
 *   cnl_conv_wgrad_workspace_bytes = slices * Cout * KH * KW * Cin * 4.  cnl_conv_wgrad_terms = rows_per_slice * W + slices: an upper
 *   bound on the fp32 additions on the path to any dw element (the chain inside a slice plus the reduce).  All three are pure host
 *   functions.  CNL_E_WORKSPACE for a null or short workspace.
 *
 * cnl_conv1x1_dgrad_nhwc_f32: dx[p][ci] = sum_co dz[p][co] * w[co][ci] (w: [Cout][Cin] dense), the input gradient of a 1x1 conv whose
 *   Cout is the head's channel count (any value >= 1: the case the forward kernels refuse as Cin of the transposed problem); Cin % 32 == 0.
 *   Exactly Cout fmaf per element, co ascending.
 */
size_t cnl_relu_grad_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int64_t cnl_relu_grad_terms(int32_t N, int32_t C, int32_t H, int32_t W);
int cnl_relu_grad_f32(const float* dy, int64_t dy_sn, int64_t dy_sc, int64_t dy_sh, int64_t dy_sw, const float* y, int32_t ldy, int32_t N, int32_t C,
                      int32_t H, int32_t W, float* dz, int32_t lddz, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int64_t cnl_conv_wgrad_slices(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW);
size_t cnl_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW);
int64_t cnl_conv_wgrad_terms(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW);
int cnl_conv_wgrad_nhwc_f32(const float* x, int32_t ldx, const float* dz, int32_t lddz, float* dw, int32_t N, int32_t H, int32_t W, int32_t Cin,
                            int32_t Cout, int32_t KH, int32_t KW, int32_t pad, void* workspace, size_t workspace_bytes, void* stream);
int cnl_conv1x1_dgrad_nhwc_f32(const float* dz, int32_t lddz, const float* w, float* dx, int32_t lddx, int32_t N, int32_t H, int32_t W, int32_t Cin,
                               int32_t Cout, void* stream);

int cnl_version(void);
/* sizeof(cnl_conv_params) / sizeof(cnl_decode_params) / sizeof(cnl_deconv_params) (which = 0 / 1 / 2), sizeof(cnl_loss_params) (which = 4) and sizeof(cnl_reid_loss_params) (which = 5; 3 is
 * unused; else 0) as the library was compiled — the structs grow at the end between ABI
 * versions: a binder (ctypes, cgo, JNI ...) compares its own struct's size before the first call (ABI v12). */
size_t cnl_sizeof_params(int32_t which);
/* Copies the calling thread's last error message (NUL-terminated) into buf; returns its length. */
size_t cnl_last_error(char* buf, size_t n);
/*
 * Page-locked host memory that the device addresses through the SAME pointer (hipHostMalloc, mapped + coherent): for small records a
 * kernel writes for the host (cnl_track_frame_f32) or reads from it (cnl_track_apply_f32's index lists).  Kernel stores are visible to
 * the host after the stream is synchronised.  Not for bulk data: every access crosses PCIe.
 */
int cnl_host_alloc(size_t bytes, void** ptr);
int cnl_host_free(void* ptr);


#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CENTERNET_GFX950_H */
