// kalman_ldl.h — the LDL' factorisation of the filter's 4 x 4 innovation covariance, shared by track_kalman.hip (the measurement update of
// cnl_track_kalman_f64) and track_costs.h (the motion gate of the gated association entries), so that both factor S with the same operations
// in the same order: the gate's squared Mahalanobis distance is taken in the metric the filter itself uses.
#pragma once

#pragma clang fp contract(off)   // one rounding per operation: tests/kalman_ref.py and tests/gate_ref.py restate every operation in numpy

namespace cnl_kalman {

// S = A + diag(r) = L D L' without square roots, column by column (include/centernet_gfx950.h: cnl_track_kalman_f64): c[i][j] = L[i][j] * d[j].
// a(i, j), i >= j, is A's element (the caller reads it from the upper triangle it keeps); only the entries L[i][j] with i > j are set.
// Returns false when a pivot of D is not finite and strictly positive (L and d are then not to be used).
template <class A>
__device__ __forceinline__ bool ldl4(const A a, const double (&r)[4], double (&L)[4][4], double (&d)[4]) {
    double c[4][4];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = j; i < 4; ++i) {
            double v = i == j ? a(i, i) + r[i] : a(i, j);
            if (j > 0) {
                double acc = c[i][0] * L[j][0];
#pragma unroll
                for (int k = 1; k < j; ++k) acc = acc + c[i][k] * L[j][k];
                v = v - acc;
            }
            c[i][j] = v;
        }
        d[j] = c[j][j];
        ok = ok && d[j] > 0.0 && d[j] < __builtin_inf();
#pragma unroll
        for (int i = j + 1; i < 4; ++i) L[i][j] = c[i][j] / d[j];
    }
    return ok;
}

}  // namespace cnl_kalman
