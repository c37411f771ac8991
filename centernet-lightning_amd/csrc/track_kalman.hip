// track_kalman.hip — the tracker's per-track Kalman filter on the device (include/centernet_gfx950.h: cnl_track_kalman_f64), so that with
// use_kalman=True the filter state (8 + 64 float64 per track) lives beside the embedding / box table and a tracking step runs no per-track
// arithmetic on the host.
//
// Replaces, per step, of centernet_lightning/models/tracker.py:
//   :243-262  Track.__init__'s KalmanFilter (state = box corners + velocities, DeepSORT-style initial covariance)
//   :281-290  Track.predict (x = Fx, P = FPF' + Q, Q from the current width / height)
//   :317-323  Track.update  (R from the current width / height, filterpy's update with the Joseph form of P)
//
// The rule — filterpy's equations specialised to F = [[I, I], [0, I]] and H = [I 0], S^-1 through an LDL' factorisation, every sum in ascending
// index order, one rounding per operation — is stated in the header and restated in numpy by tests/kalman_ref.py; the two agree bit for bit.
//
// Mapping: ONE LANE PER TRACK.  The symmetric P is 36 doubles in registers (every index below is a compile-time constant after unrolling);
// the update keeps P, the new P, K (8 x 4) and one row of (I - KH)P live.  The launch is latency-bound (a few thousand dependent float64
// operations per row, at most a few thousand rows), rows are independent, and this mapping needs no LDS, no shuffles and no scratch
// (DESIGN.md records the compiled resource usage).
#include "cnl_common.h"
#include "kalman_ldl.h"       // ldl4 (shared with track_costs.h)

#pragma clang fp contract(off)   // one rounding per operation: tests/kalman_ref.py restates every operation in numpy

namespace cnl_kalman {

// index of P[i][j] in the packed upper triangle (row-major, i <= j after the swap)
__host__ __device__ constexpr int tri(int i, int j) { return i <= j ? i * 8 - i * (i - 1) / 2 + (j - i) : j * 8 - j * (j - 1) / 2 + (i - j); }

struct State {
    double x[8];
    double p[36];
};

// BoxKalman.__init__: x = (box, 0), P = diag(std^2), std = (w, h, w, h) / 10 for the corners and / 16 for the velocities
__device__ __forceinline__ void init(State& s, const float4 b) {
    s.x[0] = (double)b.x; s.x[1] = (double)b.y; s.x[2] = (double)b.z; s.x[3] = (double)b.w;
    s.x[4] = s.x[5] = s.x[6] = s.x[7] = 0.0;
    const double w = s.x[2] - s.x[0], h = s.x[3] - s.x[1];
#pragma unroll
    for (int i = 0; i < 36; ++i) s.p[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double sd = ((i & 1) ? h : w) / (i < 4 ? 10.0 : 16.0);
        s.p[tri(i, i)] = sd * sd;
    }
}

// The measurement update with z; returns false (state untouched) when a pivot of D is not finite and strictly positive.
__device__ __forceinline__ bool update(State& s, const float4 zf) {
    const double z[4] = {(double)zf.x, (double)zf.y, (double)zf.z, (double)zf.w};
    const double w = s.x[2] - s.x[0], h = s.x[3] - s.x[1];
    double r[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double t = ((i & 1) ? h : w) / 20.0;
        r[i] = t * t;
        y[i] = z[i] - s.x[i];
    }
    // S = P[:4, :4] + diag(r) = L D L' (kalman_ldl.h: the motion gate of the association entries factors the same S the same way)
    double L[4][4], d[4];
    const bool ok = ldl4([&s](int i, int j) { return s.p[tri(i, j)]; }, r, L, d);
    // K = P[:, :4] S^-1, row by row: forward solve with L, divide by D, backward solve with L'
    double K[8][4];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        double u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = s.p[tri(m, i)];
            if (i > 0) {
                double acc = L[i][0] * u[0];
#pragma unroll
                for (int k = 1; k < i; ++k) acc = acc + L[i][k] * u[k];
                v = v - acc;
            }
            u[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = u[i] / d[i];
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double v = u[i];
            if (i < 3) {
                double acc = L[i + 1][i] * K[m][i + 1];
#pragma unroll
                for (int k = i + 2; k < 4; ++k) acc = acc + L[k][i] * K[m][k];
                v = v - acc;
            }
            K[m][i] = v;
        }
    }
    // x += K y
    double xn[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        double acc = K[m][0] * y[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) acc = acc + K[m][k] * y[k];
        xn[m] = s.x[m] + acc;
    }
    // P = (I - KH) P (I - KH)' + K R K', upper triangle: W = P - K P[:4, :] one row at a time
    double pn[36];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double W[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            double acc = K[i][0] * s.p[tri(0, j)];
#pragma unroll
            for (int k = 1; k < 4; ++k) acc = acc + K[i][k] * s.p[tri(k, j)];
            W[j] = s.p[tri(i, j)] - acc;
        }
#pragma unroll
        for (int j = i; j < 8; ++j) {
            double a = W[0] * K[j][0], b = (K[i][0] * r[0]) * K[j][0];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                a = a + W[k] * K[j][k];
                b = b + (K[i][k] * r[k]) * K[j][k];
            }
            pn[tri(i, j)] = (W[j] - a) + b;
        }
    }
    if (ok) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s.x[i] = xn[i];
#pragma unroll
        for (int i = 0; i < 36; ++i) s.p[i] = pn[i];
    }
    return ok;
}

// x = F x, P = F P F' + Q with P = [[A, B], [B', C]]: A <- (A + B') + (B + C), B <- B + C, C <- C; Q = diag(std^2), std = (w, h, w, h) / 20
// for the corners and / 160 for the velocities, from the width / height BEFORE the step
__device__ __forceinline__ void predict(State& s) {
    const double w = s.x[2] - s.x[0], h = s.x[3] - s.x[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) s.x[i] = s.x[i] + s.x[4 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j)
            s.p[tri(i, j)] = (s.p[tri(i, j)] + s.p[tri(j, 4 + i)]) + (s.p[tri(i, 4 + j)] + s.p[tri(4 + i, 4 + j)]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) s.p[tri(i, 4 + j)] = s.p[tri(i, 4 + j)] + s.p[tri(4 + i, 4 + j)];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double sd = ((i & 1) ? h : w) / (i < 4 ? 20.0 : 160.0);
        s.p[tri(i, i)] = s.p[tri(i, i)] + sd * sd;
    }
}

__global__ __launch_bounds__(64) void kalman_kernel(const double* __restrict__ x, const double* __restrict__ P, const float* __restrict__ det_box,
                                                    const int* __restrict__ src_trk, const int* __restrict__ src_det,
                                                    const int* __restrict__ flags, int T_new, double* __restrict__ new_x,
                                                    double* __restrict__ new_P, float* __restrict__ new_box, double* __restrict__ out_box,
                                                    int* __restrict__ out_status) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= T_new) return;
    const int t = src_trk[r], d = src_det[r], f = flags[r];
    State s;
    int status = 0;
    if (t >= 0 && x != nullptr) {
        const double* xo = x + (long)t * 8;
        const double* po = P + (long)t * 64;
#pragma unroll
        for (int i = 0; i < 8; ++i) s.x[i] = xo[i];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = i; j < 8; ++j) s.p[tri(i, j)] = po[i * 8 + j];
        if (d >= 0 && !update(s, *reinterpret_cast<const float4*>(det_box + (long)d * 4))) status = 1;
    } else if (t < 0 && d >= 0) {
        init(s, *reinterpret_cast<const float4*>(det_box + (long)d * 4));
    } else {      // a row without a source (an old row without an old table, or neither list names one): zeros, bit 1
#pragma unroll
        for (int i = 0; i < 8; ++i) s.x[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 36; ++i) s.p[i] = 0.0;
        status = 2;
    }
    if (d >= 0 && status != 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) new_box[(long)r * 4 + i] = (float)s.x[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out_box[(long)r * 4 + i] = s.x[i];
    out_status[r] = status;
    if (f & 1) predict(s);
    double* xn = new_x + (long)r * 8;
    double* pn = new_P + (long)r * 64;
#pragma unroll
    for (int i = 0; i < 8; ++i) xn[i] = s.x[i];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) pn[i * 8 + j] = s.p[tri(i, j)];
}

}  // namespace cnl_kalman
using namespace cnl_kalman;

extern "C" int64_t cnl_track_kalman_out_bytes(int32_t T_new) { return T_new > 0 ? 36l * T_new : 0; }

extern "C" int cnl_track_kalman_f64(const double* x, const double* P, const float* det_box, const int32_t* src_trk, const int32_t* src_det,
                                    const int32_t* flags, int32_t T_new, double* new_x, double* new_P, float* new_box, double* out_box,
                                    int32_t* out_status, void* stream) {
    CNL_REQUIRE(T_new >= 0, CNL_E_BAD_ARG, "cnl_track_kalman_f64: bad T_new");
    if (T_new == 0) return CNL_OK;
    CNL_REQUIRE(det_box && src_trk && src_det && flags && new_x && new_P && new_box && out_box && out_status, CNL_E_BAD_ARG,
                "cnl_track_kalman_f64: null pointer");
    CNL_REQUIRE((x == nullptr) == (P == nullptr), CNL_E_BAD_ARG, "cnl_track_kalman_f64: x and P come together (both null without an old table)");
    CNL_REQUIRE(new_x != x && new_P != P, CNL_E_BAD_ARG, "cnl_track_kalman_f64: the new tables must not alias the old ones");
    CNL_REQUIRE((((uintptr_t)x | (uintptr_t)P | (uintptr_t)new_x | (uintptr_t)new_P | (uintptr_t)out_box) & 7) == 0, CNL_E_BAD_ARG,
                "cnl_track_kalman_f64: x, P, new_x, new_P and out_box must be 8-byte aligned");
    CNL_REQUIRE(((uintptr_t)det_box & 15) == 0, CNL_E_BAD_ARG, "cnl_track_kalman_f64: det_box must be 16-byte aligned");
    CNL_REQUIRE((((uintptr_t)src_trk | (uintptr_t)src_det | (uintptr_t)flags | (uintptr_t)new_box | (uintptr_t)out_status) & 3) == 0, CNL_E_BAD_ARG,
                "cnl_track_kalman_f64: src_trk, src_det, flags, new_box and out_status must be 4-byte aligned");
    hipLaunchKernelGGL(kalman_kernel, dim3((unsigned)((T_new + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x, P, det_box, src_trk, src_det, flags,
                       T_new, new_x, new_P, new_box, out_box, out_status);
    return cnl::check_launch("track kalman_kernel");
}
