// Device primitives shared by every matrix-core convolution kernel (winograd*.hip, conv_mfma.hip / conv_f16x2.hip through conv_args.h, stem*.hip,
// pointwise.hip, tools/experiments/winograd*.hip): vector types, buffer loads / stores / LDS DMA, the fp16 MFMA, the fp16-split primitives.
// One definition each; a kernel file says `using namespace cnl_dev;` inside its own namespace and keeps only what is its own (tile constants,
// Args / State, schedules, trace macros, and helpers with another signature or instruction: those hide the names here).
#pragma once
#include "cnl_common.h"

namespace cnl_dev {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr unsigned OOB = 0xFFFFFFF0u;   // voffset that is always >= num_records -> a load returns zeros (DMA writes zeros), a store is dropped

// every wave's LDS traffic has landed, then the workgroup meets (no vmcnt wait: global loads stay in flight across it)
#define CNL_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Buffer access: `bytes` = num_records of the descriptor, voffset per lane, soffset uniform.  AUX = cache policy (0: default, 1 = sc0, 2 = nt,
// 16 = sc1): a template parameter, so that a file's A/B macro (W9_NT_Y, W5_NT_X ...) or CNL_NT_STORES picks it per call site.
// amdgcn builtins are wrapped in device functions of their own (here: templates over the policy ONLY, checked against the host pass — every
// kernel keeps its host stub): called with template-dependent arguments directly inside a kernel template they make hipcc's host pass
// silently drop the kernel's host stub.
template <int AUX = 0>
__device__ __forceinline__ void dma16(const void* base, unsigned bytes, char* lds_dst, unsigned voffset, unsigned soffset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_dst, 16, voffset, soffset, 0, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ u32x4 buf_load16(const void* base, unsigned bytes, unsigned voffset, unsigned soffset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
    return (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, soffset, AUX);
}
template <int AUX = CNL_NT_STORES>
__device__ __forceinline__ void buf_store16(f32x4 v, float* base, unsigned bytes, unsigned voffset, unsigned soffset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, voffset, soffset, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ float buf_load(const float* base, unsigned bytes, unsigned voffset, unsigned soffset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voffset, soffset, AUX));
}
template <int AUX = CNL_NT_STORES>
__device__ __forceinline__ void buf_store(float v, float* base, unsigned bytes, unsigned voffset, unsigned soffset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, voffset, soffset, AUX);
}
__device__ __forceinline__ f32x4 lds_f4(const char* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ u32x4 lds_u4(const char* p) { return *reinterpret_cast<const u32x4*>(p); }

// D[32 x 32] += A[32 x 16] B[16 x 32] on the fp16 matrix cores, fp32 accumulation
__device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_zero() {        // 16 zeroed accumulator registers from ONE instruction
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const u32x4 zz = {0u, 0u, 0u, 0u};
    return mfma16(zz, zz, z);
}

// ---- the fp16 split: the arithmetic contract of the whole fp16-split class -------------------------------------------------------------
// With a power-of-two scale S per tensor or image (max |x S| in [2^13, 2^14), exact), x S = hi + lo with hi = RN16(x S), lo = RZ16(x S - hi)
// represents x to 2^-22 relative (down to 2^-17 of the tensor's maximum; below that the ABSOLUTE error stays <= 2^-25 / S, i.e. 2^-38 of the
// maximum), and the three terms  hi lo' + lo hi' + hi hi'  on the fp16 matrix cores (fp32 accumulation) leave out lo lo' <= 2^-22 |x y|.
// Measured on MI355X (tools/bf16x3_probe.hip, K = 2304): max |err| 7.7e-6 / rms 9.2e-7 against 1.27e-5 / 1.36e-6 for the fp32 MFMA and
// 8.0e-6 / 1.33e-6 for the six-term bf16 split; fp16 subnormals run at full MFMA rate and are not flushed.
// The mixed-precision fma does the scaling, the rounding and the exact residual:  hi = v_fma_mixlo/hi_f16(v, S, 0),  r = v_fma_mix_f32(v, S, -hi)
// = v S - hi EXACTLY (one fused multiply-subtract: |r| <= half an fp16 ulp of hi),  lo = v_cvt_pkrtz_f16_f32(r0, r1) at the call sites.
// The four primitives work on a channel pair (v0, v1) packed into one register.  Inline asm on purpose in the Winograd kernels, which place
// each of them in an MFMA slice of their static schedules (VALU-only: v_fma_mix*); kernels that leave the placement to the compiler use
// split2 / split8 below.
__device__ __forceinline__ unsigned split_hi_lo(float v0, float S) {            // RN16(v0 S) in the low half
    unsigned pk;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(pk) : "v"(v0), "v"(S));
    return pk;
}
__device__ __forceinline__ unsigned split_hi_hi(unsigned pk, float v1, float S) {   // ... and RN16(v1 S) in the high half
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(pk) : "v"(v1), "v"(S));
    return pk;
}
__device__ __forceinline__ float split_res_lo(float v, float S, unsigned pk) {   // v S - (low half of pk)
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(v), "v"(S), "v"(pk));
    return r;
}
__device__ __forceinline__ float split_res_hi(float v, float S, unsigned pk) {   // v S - (high half of pk)
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(v), "v"(S), "v"(pk));
    return r;
}
// The same split of a pair in plain C: (v0, v1) S -> hi pair (RN16, packed) and lo pair (RZ16 of the exact residuals, packed).  The compiler
// folds it into v_fma_mixlo/mixhi_f16, v_fma_mix_f32 and v_cvt_pkrtz_f16_f32, and — unlike with inline asm — its hazard recognizer then sees
// VALU instructions and keeps the two wait states gfx950 needs between a VALU write and an MFMA reading that register.
__device__ __forceinline__ void split2(float v0, float v1, float S, unsigned& hi, unsigned& lo) {
    const _Float16 h0 = (_Float16)__builtin_fmaf(v0, S, 0.f), h1 = (_Float16)__builtin_fmaf(v1, S, 0.f);
    const float r0 = __builtin_fmaf(v0, S, -(float)h0), r1 = __builtin_fmaf(v1, S, -(float)h1);
    const f16x2 hv = {h0, h1};
    hi = __builtin_bit_cast(unsigned, hv);
    lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
}
__device__ __forceinline__ void split8(const f32x4& v0, const f32x4& v1, float S, u32x4& hi, u32x4& lo) {
    unsigned h[4], l[4];
    split2(v0[0], v0[1], S, h[0], l[0]);
    split2(v0[2], v0[3], S, h[1], l[1]);
    split2(v1[0], v1[1], S, h[2], l[2]);
    split2(v1[2], v1[3], S, h[3], l[3]);
    hi = u32x4{h[0], h[1], h[2], h[3]};
    lo = u32x4{l[0], l[1], l[2], l[3]};
}
// the power of two that puts a tensor of maximum magnitude mx into [2^13, 2^14)  (1 for 0 / Inf / NaN maxima)
__device__ __forceinline__ float pow2_scale(float mx) {
    float S = 1.f;
    if (mx > 0.f && mx < __builtin_inff()) {
        int e;
        (void)__builtin_frexpf(mx, &e);            // 2^(e-1) <= mx < 2^e
        e = 14 - e;
        S = __builtin_ldexpf(1.f, e < -60 ? -60 : (e > 60 ? 60 : e));
    }
    return S;
}

// the lane id from the hardware (2 VALU) on an opaque input: per-lane values derived from it are computed where they are used instead
// of at kernel entry, from where they would stay live across the chunk loop
__device__ __forceinline__ int lane_now() {
    unsigned z = 0;
    asm volatile("" : "+v"(z));
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}

}  // namespace cnl_dev
