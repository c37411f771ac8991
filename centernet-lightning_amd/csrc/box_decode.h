// The fp32 box decode rule (reference centernet.py:278-303), shared by the decode (decode.hip: the fused top-k path and the standalone gather) and
// by the validation loss's box samples (det_loss.hip): ONE device function, so the loss is measured on exactly the boxes the decode emits.
#pragma once
#include <hip/hip_runtime.h>

namespace cnl {

// bp: the pixel's first box value, bsc the channel stride (elements); (xi, yi) the pixel; bo <- x1 y1 x2 y2.  One rounding per operation, like ATen.
__device__ __forceinline__ void decode_box(const float* bp, long bsc, int xi, int yi, int W, int H, int normalize, int box_log,
                                           float mult, float stride, float* bo) {
#pragma clang fp contract(off)
    const float cx = (float)xi + 0.5f, cy = (float)yi + 0.5f;
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v = bp[(long)j * bsc];
        if (box_log) v = expf(v);
        v = v * mult;
        g[j] = fmaxf(v, 0.f);
    }
    float x1 = cx - g[0], y1 = cy - g[1], x2 = cx + g[2], y2 = cy + g[3];
    if (normalize) {
        const float fw = (float)W, fh = (float)H;
        x1 = x1 / fw; x2 = x2 / fw; y1 = y1 / fh; y2 = y2 / fh;
    } else {
        x1 *= stride; y1 *= stride; x2 *= stride; y2 *= stride;
    }
    bo[0] = x1; bo[1] = y1; bo[2] = x2; bo[3] = y2;
}

}  // namespace cnl
