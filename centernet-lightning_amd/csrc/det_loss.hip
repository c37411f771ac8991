// det_loss.hip — the validation value of the detection losses (reference models/centernet.py:123-200 compute_loss / update_heatmap,
// losses/heatmap_losses.py, losses/box_losses.py) on the device: Gaussian targets, heatmap loss and the 3x3 centre-sampled box loss of a
// batch in four launches, the logits read once, no N x C x H x W target tensor unless the caller asks for it.  The rule is stated in
// include/centernet_gfx950.h and restated in numpy in tests/loss_ref.py.  The gradient of that value with respect to the logits and the box_2d
// values (cnl_detection_loss_grad_f32, the second half of this file; tests/loss_grad_ref.py) is analytic: no double backward (the re-ID loss of the tracking model is csrc/reid_loss.hip).
//
//   record_kernel    one thread per target slot: box -> (cx, cy, rx, ry, the two fp32 Gaussian denominators, label, state), all float64
//                    as the reference's host code computes them.  Slots at or beyond count[n] are never read.
//   heatmap_kernel   the hot path.  A workgroup owns a tile of pixels of one image over ALL classes (loss_common.h: Tile).  It stages the
//                    image's records whose window touches the tile in LDS in slot order (stage, over loss_common.h's stage_pass; an image
//                    of at most PASS_SLOTS boxes is staged once), reads each logit exactly once, forms the element's target in registers
//                    (the maximum over the staged records of its class), and adds the element's float64 loss term to a per-thread sum in
//                    element order; the workgroup folds its 256 sums in a fixed tree into ONE float64 partial.  Three element orders
//                    (loss_common.h: element): channel stride 1 (the engine's channels-last maps), W stride 1 (planes, classes outermost),
//                    and the plane order with free strides.
//   sample_kernel    one workgroup per image: the up to nine box samples of every counted record, decoded by the decode's own device
//                    function (box_decode.h), the loss per sample in float64, summed per thread in slot order and folded in a fixed tree.
//   finish_kernel    one workgroup: a wave per image folds the image's tile partials (lane stripes in index order, then a fixed tree) into
//                    its row; thread 0 then adds the rows in image order into the three totals.
// No floating-point atomics, no atomics at all: an image's row is a function of that image alone.  Nothing here synchronises the device.
#include "loss_common.h"

#pragma clang fp contract(off)   // one rounding per operation

#include "box_decode.h"

namespace cnl_det_loss {

using namespace cnl_loss;

constexpr int MAX_C = 1 << 16;
constexpr int RADIUS_CAP = 1 << 24;                // window radii beyond any map are clamped here (the Gaussian's width is not)

struct alignas(16) Rec {
    int cx, cy, rx, ry;
    float den_x, den_y;        // fl32(2 sx sx), fl32(2 sy sy)
    int label;
    int state;                 // 0 skipped, 1 counted
};
static_assert(sizeof(Rec) == 32, "record layout");

struct Sections {              // the workspace: records | tile partials | per-image sample results
    size_t rec, part, img, total;
};
inline Sections sections(int N, int Gmax, int H, int W) {
    Sections s;
    s.rec = 0;
    s.part = s.rec + (size_t)N * Gmax * sizeof(Rec);
    s.img = s.part + (size_t)N * tiles_x(W) * tiles_y(H) * sizeof(double);
    s.total = s.img + (size_t)N * 4 * sizeof(double);
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- records
__device__ __forceinline__ double cornernet_radius(double w, double h, double mo) {      // centernet.py:38-58, operation by operation
    const double b1 = h + w;
    const double c1 = w * h * (1.0 - mo) / (1.0 + mo);
    const double r1 = (b1 - sqrt(b1 * b1 - 4.0 * c1)) / 2.0;
    const double b2 = 2.0 * (h + w);
    const double c2 = (1.0 - mo) * w * h;
    const double r2 = (b2 - sqrt(b2 * b2 - 16.0 * c2)) / 8.0;
    const double a3 = 4.0 * mo;
    const double b3 = -2.0 * mo * (h + w);
    const double c3 = (mo - 1.0) * w * h;
    const double r3 = (b3 + sqrt(b3 * b3 - 4.0 * a3 * c3)) / (2.0 * a3);
    double r = r1;                                           // Python's min(r1, r2, r3): the first of the smallest
    if (r2 < r) r = r2;
    if (r3 < r) r = r3;
    return r;
}

__global__ __launch_bounds__(THREADS) void record_kernel(const double* __restrict__ boxes, const long long* __restrict__ labels,
                                                         const int* __restrict__ count, int N, int Gmax, int C, int H, int W, double stride,
                                                         int method, double param, Rec* __restrict__ rec) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (long)N * Gmax) return;
    const int n = (int)(i / Gmax), s = (int)(i - (long)n * Gmax);
    if (s >= min(max(count[n], 0), Gmax)) return;            // never read, never staged
    const double* const b = boxes + i * 4;
    const double x = b[0] / stride, y = b[1] / stride, w = b[2] / stride, h = b[3] / stride;
    const long long label = labels[i];
    Rec r;
    r.cx = r.cy = r.rx = r.ry = 0; r.den_x = r.den_y = 1.f; r.label = -1; r.state = 0;
    const double cx = rint(x + w / 2.0), cy = rint(y + h / 2.0);      // numpy's round: ties to even
    double rx, ry;
    if (method == 0) rx = ry = cornernet_radius(w, h, param);
    else if (method == 1) { rx = w / 2.0 * param; ry = h / 2.0 * param; }
    else rx = ry = param;
    rx = rint(rx); ry = rint(ry);
    // (every comparison is false for a NaN: a non-finite number anywhere skips the box)
    const bool finite = fabs(x) < __builtin_inf() && fabs(y) < __builtin_inf() && w < __builtin_inf() && h < __builtin_inf() &&
                        fabs(rx) < __builtin_inf() && fabs(ry) < __builtin_inf();
    if (finite && w >= 0.0 && h >= 0.0 && cx >= 0.0 && cx <= (double)W && cy >= 0.0 && cy <= (double)H && label >= 0 && label < C) {
        rx = fmax(rx, 0.0); ry = fmax(ry, 0.0);
        const double sx = rx / 3.0 + 1.0 / 6.0, sy = ry / 3.0 + 1.0 / 6.0;
        r.cx = (int)cx; r.cy = (int)cy;
        r.rx = (int)fmin(rx, (double)RADIUS_CAP); r.ry = (int)fmin(ry, (double)RADIUS_CAP);
        r.den_x = (float)(2.0 * (sx * sx)); r.den_y = (float)(2.0 * (sy * sy));
        r.label = (int)label;
        r.state = 1;
    }
    rec[i] = r;
}

// ---------------------------------------------------------------------------------------------------------------- heatmap
struct HeatArgs {                                  // of heatmap_kernel (the value) and heat_grad_kernel (its gradient)
    const float* heat; long sn, sc, sh, sw;        // NULL (value only): targets only
    float* out; long on, oc, oh, ow;               // the value: the target map, NULL: never written; the gradient: the heatmap gradient
    const Rec* rec;
    const int* count;
    double* part;                                  // the value: a float64 partial per tile
    const double* counts;                          // the gradient: num_dets, num_boxes
    const double* scales;                          // the gradient: s_heat, s_box; NULL: 1, 1
    int C, H, W, Gmax, tx;
    int loss;                                      // 0 cornernet_focal, 1 quality
    int alpha_is_2, beta_is_4, beta_is_2;
    double alpha, beta;
};

// one pass: the records of slots s0 .. s0 + PASS_SLOTS - 1 whose window touches the tile, compacted into s_rec in slot order -> how many
__device__ __forceinline__ int stage(const Rec* __restrict__ recs, int s0, int M, const Tile& t, Rec* s_rec, int* s_cnt) {
    const int x0 = t.x0, y0 = t.y0, x1 = t.x1, y1 = t.y1;
    return stage_pass(s0, M, s_rec, s_cnt, [=](int s, Rec& r) {
        r = recs[s];
        // (a centre ON cx == W or cy == H still renders the part of its window that lies inside the map, as the reference's slices do)
        return r.state != 0 && r.cx - r.rx < x1 && r.cx + r.rx >= x0 && r.cy - r.ry < y1 && r.cy + r.ry >= y0;
    });
}

__device__ __forceinline__ float target_of(const Rec* s_rec, int cnt, int x, int y, int c, float t) {
    for (int j = 0; j < cnt; ++j) {
        const Rec r = s_rec[j];                               // the same address in every lane: a broadcast
        const int dx = x - r.cx, dy = y - r.cy;
        if (r.label == c && abs(dx) <= r.rx && abs(dy) <= r.ry) {
            const float g = (float)(dx * dx) / r.den_x + (float)(dy * dy) / r.den_y;
            float v = (float)exp(-(double)g);
            if (v < 1.1920928955078125e-07f) v = 0.f;         // the reference's cut at eps * max, max == 1
            t = fmaxf(t, v);
        }
    }
    return t;
}

// t[k] <- the target of element (x[k], y, c[k]) over all M records of the image (0 where !inside).  A single pass was staged once before the
// element loop (cnt) and stays; several passes are restaged here, by every thread of the workgroup (stage_pass's barriers).
template <int PER>
__device__ __forceinline__ void targets_of(const Rec* __restrict__ recs, int M, int passes, const Tile& tile, Rec* s_rec, int* s_cnt, int& cnt, bool inside,
                                           const int (&x)[PER], int y, const int (&c)[PER], float (&t)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; ++k) t[k] = 0.f;
    if (passes <= 1) {
        if (inside) {
#pragma unroll
            for (int k = 0; k < PER; ++k) t[k] = target_of(s_rec, cnt, x[k], y, c[k], 0.f);
        }
    } else {
        for (int p = 0; p < passes; ++p) {
            cnt = stage(recs, p * PASS_SLOTS, M, tile, s_rec, s_cnt);
            if (inside) {
#pragma unroll
                for (int k = 0; k < PER; ++k) t[k] = target_of(s_rec, cnt, x[k], y, c[k], t[k]);
            }
        }
    }
}

__device__ __forceinline__ double pow_small(double v, double e, int is2, int is4) {
    if (is2) return v * v;
    if (is4) { const double v2 = v * v; return v2 * v2; }
    return pow(v, e);
}

// p = 1 / (1 + exp(-x)) without the overflow, and log1p(exp(-|x|))
struct Sigmoid { double p, l1p; };
__device__ __forceinline__ Sigmoid sigmoid_of(double x) {
    const double e = exp(-fabs(x));
    const double l1p = log1p(e);
    const double inv = 1.0 / (1.0 + e);
    return {x >= 0.0 ? inv : e * inv, l1p};
}

__device__ __forceinline__ double heat_term(const HeatArgs& a, float logit, float t) {
    const double x = (double)logit, td = (double)t;
    const Sigmoid s = sigmoid_of(x);
    const double p = s.p, l1p = s.l1p;
    if (a.loss == 0) {
        const double pos = t == 1.f ? -pow_small(1.0 - p, a.alpha, a.alpha_is_2, 0) * (fmin(x, 0.0) - l1p) : 0.0;
        const double neg = -pow_small(p, a.alpha, a.alpha_is_2, 0) * (fmin(-x, 0.0) - l1p) * pow_small(1.0 - td, a.beta, 0, a.beta_is_4);
        return pos + neg;
    }
    return pow_small(fabs(td - p), a.beta, a.beta_is_2, 0) * (fmax(x, 0.0) - x * td + l1p);
}

template <int LAYOUT>
__global__ __launch_bounds__(THREADS) void heatmap_kernel(const HeatArgs a) {
    __shared__ Rec s_rec[PASS_SLOTS];
    __shared__ int s_cnt[WAVES];
    __shared__ double s_part[WAVES];
    const Tile tile(blockIdx.x, a.tx, a.H, a.W);
    const int M = min(max(a.count[tile.n], 0), a.Gmax);
    const Rec* const recs = a.rec + (long)tile.n * a.Gmax;
    const int passes = (M + PASS_SLOTS - 1) / PASS_SLOTS;
    const long sw = LAYOUT == LAYOUT_PLANE ? 1 : a.sw, sc = LAYOUT == LAYOUT_CMINOR ? 1 : a.sc;
    const float* const heat = a.heat ? a.heat + (long)tile.n * a.sn : nullptr;
    float* const tmap = a.out ? a.out + (long)tile.n * a.on : nullptr;

    int cnt = passes == 1 ? stage(recs, 0, M, tile, s_rec, s_cnt) : 0;
    double acc = 0.0;
    for (int step = 0; step < a.C; ++step) {
        const Elem e = element(LAYOUT == LAYOUT_CMINOR, tile, step, a.C);
        const int x[1] = {e.x}, c[1] = {e.c}, y = e.y;
        const bool inside = tile.holds(e.x, y);
        float logit = 0.f;
        if (inside && heat) logit = heat[(long)e.c * sc + (long)y * a.sh + (long)e.x * sw];      // requested before the target's arithmetic
        float t[1];
        targets_of(recs, M, passes, tile, s_rec, s_cnt, cnt, inside, x, y, c, t);
        if (inside) {
            if (tmap) tmap[(long)e.c * a.oc + (long)y * a.oh + (long)e.x * a.ow] = t[0];
            if (heat) acc += heat_term(a, logit, t[0]);
        }
    }
    const double total = block_sum_fixed(acc, s_part);
    if (threadIdx.x == 0) a.part[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------------------------- box samples
__device__ __forceinline__ double box_term(int kind, const float* pf, const float* tf) {      // losses/box_losses.py on (pred, target), float64
    double p[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { p[j] = (double)pf[j]; t[j] = (double)tf[j]; }
    if (kind <= 1) {                                          // l1, smooth_l1 (beta 1): the four coordinates in order
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = fabs(p[j] - t[j]);
            s += kind == 0 ? d : (d < 1.0 ? 0.5 * d * d : d - 0.5);
        }
        return s;
    }
    const double eps = 1e-8;
    const double area1 = (p[2] - p[0]) * (p[3] - p[1]), area2 = (t[2] - t[0]) * (t[3] - t[1]);
    const double iw = fmax(fmin(p[2], t[2]) - fmax(p[0], t[0]), 0.0), ih = fmax(fmin(p[3], t[3]) - fmax(p[1], t[1]), 0.0);
    const double inter = iw * ih;
    const double uni = area1 + area2 - inter;
    const double iou = inter / (uni + eps);
    if (kind == 2) return 1.0 - iou;
    const double ex1 = fmin(p[0], t[0]), ey1 = fmin(p[1], t[1]), ex2 = fmax(p[2], t[2]), ey2 = fmax(p[3], t[3]);
    if (kind == 3) {
        const double enclosing = (ex2 - ex1) * (ey2 - ey1);
        const double giou = iou - (1.0 - uni / enclosing);
        return 1.0 - giou;
    }
    const double ew = ex2 - ex1, eh = ey2 - ey1;
    const double diagonal = ew * ew + eh * eh;
    const double ddx = (t[0] + t[2]) / 2.0 - (p[0] + p[2]) / 2.0, ddy = (t[1] + t[3]) / 2.0 - (p[1] + p[3]) / 2.0;
    const double penalty = (ddx * ddx + ddy * ddy) / diagonal;
    if (kind == 4) return 1.0 - iou + penalty;
    const double w1 = p[2] - p[0], h1 = p[3] - p[1], w2 = t[2] - t[0], h2 = t[3] - t[1];
    const double angle = (atan(w1 / (h1 + eps)) - atan(w2 / (h2 + eps))) * 2.0 / 3.141592653589793;
    const double v = angle * angle;
    const double alpha = v / (1.0 - iou + v + eps);
    return 1.0 - iou + penalty + alpha * v;
}

__global__ __launch_bounds__(THREADS) void sample_kernel(const float* __restrict__ box, long sn, long sc, long sh, long sw,
                                                         const double* __restrict__ gt_boxes, const int* __restrict__ count,
                                                         const Rec* __restrict__ rec, int Gmax, int H, int W, int kind, int box_log, float mult,
                                                         float stride, double* __restrict__ img) {
    __shared__ double s_part[WAVES];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int M = min(max(count[n], 0), Gmax);
    double sum = 0.0, dets = 0.0, samples = 0.0, skipped = 0.0;      // (counts below 2^53: exact)
    for (int s = tid; s < M; s += THREADS) {
        const Rec r = rec[(long)n * Gmax + s];
        if (r.state == 0) { skipped += 1.0; continue; }
        dets += 1.0;
        const double* const b = gt_boxes + ((long)n * Gmax + s) * 4;
        const float target[4] = {(float)b[0], (float)b[1], (float)(b[0] + b[2]), (float)(b[1] + b[3])};
        for (int X = r.cx - 1; X <= r.cx + 1; ++X) {          // itertools.product(cxs, cys): x outer
            if (X < 0 || X > W - 1) continue;
            for (int Y = r.cy - 1; Y <= r.cy + 1; ++Y) {
                if (Y < 0 || Y > H - 1) continue;
                samples += 1.0;
                if (box) {
                    float pred[4];
                    cnl::decode_box(box + (long)n * sn + (long)Y * sh + (long)X * sw, sc, X, Y, W, H, 0, box_log, mult, stride, pred);
                    sum += box_term(kind, pred, target);
                }
            }
        }
    }
    sum = block_sum_fixed(sum, s_part);
    dets = block_sum_fixed(dets, s_part);
    samples = block_sum_fixed(samples, s_part);
    skipped = block_sum_fixed(skipped, s_part);
    if (tid == 0) {
        double* const o = img + (long)n * 4;
        o[0] = sum; o[1] = dets; o[2] = samples; o[3] = skipped;
    }
}

// ---------------------------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(THREADS) void finish_kernel(const double* __restrict__ part, const double* __restrict__ img, int N, int tiles,
                                                         double w_heat, double w_box, double* __restrict__ per_image,
                                                         double* __restrict__ totals, int* __restrict__ skipped) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int n = wave; n < N; n += WAVES) {
        double s = 0.0;
        for (int i = lane; i < tiles; i += 64) s += part[(long)n * tiles + i];      // a lane's stripe in index order
        s = wave_sum_fixed(s);
        if (lane == 0) {
            double* const row = per_image + (long)n * 4;
            row[0] = s; row[1] = img[(long)n * 4]; row[2] = img[(long)n * 4 + 1]; row[3] = img[(long)n * 4 + 2];
        }
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double heat = 0.0, box = 0.0, dets = 0.0, samples = 0.0, skip = 0.0;
        for (int n = 0; n < N; ++n) {                         // image order
            const volatile double* const row = per_image + (long)n * 4;
            heat += row[0]; box += row[1]; dets += row[2]; samples += row[3];
            skip += img[(long)n * 4 + 3];
        }
        const double h = heat / fmax(1.0, dets), b = box / fmax(1.0, samples);
        totals[0] = h; totals[1] = b; totals[2] = h * w_heat + b * w_box;
        skipped[0] = (int)skip;
    }
}

}  // namespace cnl_det_loss

// ================================================================================================================ gradient
// cnl_detection_loss_grad_f32: d(s_heat heatmap_loss + s_box box_2d_loss) / d(logits, box_2d), the rule of include/centernet_gfx950.h.
//   record_kernel        as above.
//   count_kernel         one workgroup: num_dets, num_boxes and skipped of the BATCH (integers: exact in any order), which both gradients divide by.
//   heat_grad_kernel     the hot path: the forward's tile ownership, staging and register targets (Tile, targets_of); every element's derivative in
//                        float64, rounded once, no reduction.  The element order follows the GRADIENT's strides (the write stream): channel stride 1 (and, where
//                        both maps are packed channels-last and 16-byte aligned, four consecutive elements of a tile row per lane: one 16-byte
//                        load and one 16-byte store), W stride 1, or the plane order with free strides.  The logits are read by their own strides.
//   box_grad_kernel      a workgroup per tile of one image, a thread per pixel: the image's counted records whose 3 x 3 sample neighbourhood
//                        touches the tile are staged (stage_pass) in slot order with their slot; a thread adds the contribution of every staged
//                        record that samples its pixel, in slot order, and stores its four values once (0 where none does).
namespace cnl_det_loss {

constexpr size_t COUNT_BYTES = 16;                 // num_dets, num_boxes (float64)

inline size_t grad_sections_total(int N, int Gmax) { return (size_t)N * Gmax * sizeof(Rec) + COUNT_BYTES; }

__global__ __launch_bounds__(THREADS) void count_kernel(const Rec* __restrict__ rec, const int* __restrict__ count, int N, int Gmax, int H, int W,
                                                        double* __restrict__ counts, int* __restrict__ skipped) {
    __shared__ double s_part[WAVES];
    double dets = 0.0, samples = 0.0, skip = 0.0;             // (integers below 2^53: exact, the order does not matter)
    const long slots = (long)N * Gmax;
    for (long i = threadIdx.x; i < slots; i += THREADS) {
        const int n = (int)(i / Gmax), s = (int)(i - (long)n * Gmax);
        if (s >= min(max(count[n], 0), Gmax)) continue;
        const Rec r = rec[i];
        if (r.state == 0) { skip += 1.0; continue; }
        dets += 1.0;
        const int nx = min(r.cx + 1, W - 1) - max(r.cx - 1, 0) + 1, ny = min(r.cy + 1, H - 1) - max(r.cy - 1, 0) + 1;
        samples += (double)(nx * ny);
    }
    dets = block_sum_fixed(dets, s_part);
    samples = block_sum_fixed(samples, s_part);
    skip = block_sum_fixed(skip, s_part);
    if (threadIdx.x == 0) { counts[0] = dets; counts[1] = samples; skipped[0] = (int)skip; }
}

// d(heat_term) / d(logit): p and log1p(exp(-|x|)) are heat_term's (sigmoid_of); the target and the [t == 1] weight are constants
__device__ __forceinline__ double heat_dterm(const HeatArgs& a, float logit, float t) {
    const double x = (double)logit, td = (double)t;
    const Sigmoid s = sigmoid_of(x);
    const double p = s.p, l1p = s.l1p;
    const double q = 1.0 - p, pq = p * q;                     // dp/dx = p (1 - p)
    if (a.loss == 0) {
        const double ls = fmin(x, 0.0) - l1p, lsn = fmin(-x, 0.0) - l1p;      // d ls/dx = 1 - p, d lsn/dx = -p
        double pos = 0.0;
        if (t == 1.f) {
            const double dq = a.alpha_is_2 ? 2.0 * q : a.alpha * pow(q, a.alpha - 1.0);
            pos = dq * pq * ls - pow_small(q, a.alpha, a.alpha_is_2, 0) * q;
        }
        const double dp = a.alpha_is_2 ? 2.0 * p : a.alpha * pow(p, a.alpha - 1.0);
        const double neg = (pow_small(p, a.alpha, a.alpha_is_2, 0) * p - dp * pq * lsn) * pow_small(1.0 - td, a.beta, 0, a.beta_is_4);
        return pos + neg;
    }
    const double d = td - p, ad = fabs(d);
    if (d == 0.0) return 0.0;                                 // |t - p|^beta: derivative 0 at t == p
    const double sg = d > 0.0 ? 1.0 : -1.0;
    const double ce = fmax(x, 0.0) - x * td + l1p;            // d ce/dx = p - t
    const double dm = a.beta_is_2 ? 2.0 * ad : a.beta * pow(ad, a.beta - 1.0);
    return pow_small(ad, a.beta, a.beta_is_2, 0) * (p - td) - sg * (dm * pq) * ce;
}

// VEC4: LAYOUT_CMINOR with both maps packed channels-last (pixel stride C, everything else a multiple of 4 elements, 16-byte aligned bases)
template <int LAYOUT, bool VEC4>
__global__ __launch_bounds__(THREADS) void heat_grad_kernel(const HeatArgs a) {
    constexpr int PER = VEC4 ? 4 : 1;
    __shared__ Rec s_rec[PASS_SLOTS];
    __shared__ int s_cnt[WAVES];
    const int tid = threadIdx.x;
    const Tile tile(blockIdx.x, a.tx, a.H, a.W);
    const int x0 = tile.x0, y0 = tile.y0, x1 = tile.x1, y1 = tile.y1;
    const long gw = LAYOUT == LAYOUT_PLANE ? 1 : a.ow, gc = LAYOUT == LAYOUT_CMINOR ? 1 : a.oc;
    const float* const heat = a.heat + (long)tile.n * a.sn;
    float* const grad = a.out + (long)tile.n * a.on;
    const double scale = (a.scales ? a.scales[0] : 1.0) / fmax(1.0, a.counts[0]);

    const int M = min(max(a.count[tile.n], 0), a.Gmax);
    const Rec* const recs = a.rec + (long)tile.n * a.Gmax;
    const int passes = (M + PASS_SLOTS - 1) / PASS_SLOTS;
    int cnt = passes == 1 ? stage(recs, 0, M, tile, s_rec, s_cnt) : 0;
    const int steps = VEC4 ? (a.C + 3) / 4 : a.C;                            // the same in every thread: the barriers of a multi-pass step are uniform
    for (int step = 0; step < steps; ++step) {
        int x[PER], y, c[PER];
        bool inside;
        unsigned j0 = 0;
        if (VEC4) {                                           // lanes along the 16-byte groups of a tile row, then along y
            const unsigned g = (unsigned)step * THREADS + (unsigned)tid, per_row = (unsigned)TILE_W * (unsigned)a.C / 4;
            const unsigned yy = g / per_row;
            j0 = (g - yy * per_row) * 4;
            y = y0 + (int)yy;
            inside = yy < (unsigned)TILE_H && y < y1 && j0 < (unsigned)(x1 - x0) * (unsigned)a.C;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const unsigned xx = (j0 + k) / (unsigned)a.C;
                x[k] = x0 + (int)xx; c[k] = (int)(j0 + k - xx * (unsigned)a.C);
            }
        } else {
            const Elem e = element(LAYOUT == LAYOUT_CMINOR, tile, step, a.C);
            x[0] = e.x; y = e.y; c[0] = e.c;
            inside = tile.holds(e.x, y);
        }
        float logit[PER], t[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) logit[k] = 0.f;
        if (inside) {                                         // requested before the target's arithmetic
            if (VEC4) {
                const float4 v = *reinterpret_cast<const float4*>(heat + (long)y * a.sh + (long)x0 * a.C + (long)j0);
                logit[0] = v.x; if (PER > 1) { logit[1 % PER] = v.y; logit[2 % PER] = v.z; logit[3 % PER] = v.w; }
            } else {
                logit[0] = heat[(long)c[0] * a.sc + (long)y * a.sh + (long)x[0] * a.sw];
            }
        }
        targets_of(recs, M, passes, tile, s_rec, s_cnt, cnt, inside, x, y, c, t);
        if (inside) {
            float o[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) o[k] = (float)(scale * heat_dterm(a, logit[k], t[k]));
            if (VEC4) {
                float4 v;
                v.x = o[0]; v.y = o[1 % PER]; v.z = o[2 % PER]; v.w = o[3 % PER];
                *reinterpret_cast<float4*>(grad + (long)y * a.oh + (long)x0 * a.C + (long)j0) = v;
            } else {
                grad[(long)c[0] * gc + (long)y * a.oh + (long)x[0] * gw] = o[0];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- box gradient
// d max(a, b) / da and d min(a, b) / da as torch's autograd takes them: half on a tie
__device__ __forceinline__ double d_max(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double d_min(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }

// d(box_term) / d(pred): g <- the four derivatives, float64 on the fp32 boxes; non-differentiable points as torch's autograd takes them
__device__ __forceinline__ void box_dterm(int kind, const float* pf, const float* tf, double* g) {
    double p[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { p[j] = (double)pf[j]; t[j] = (double)tf[j]; }
    if (kind <= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = p[j] - t[j];
            const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);      // |d|: derivative 0 at 0
            g[j] = kind == 0 ? sg : (fabs(d) < 1.0 ? d : sg);              // smooth_l1: the quadratic branch for |d| < 1
        }
        return;
    }
    const double eps = 1e-8;
    const double w1 = p[2] - p[0], h1 = p[3] - p[1];
    const double area1 = w1 * h1, area2 = (t[2] - t[0]) * (t[3] - t[1]);
    const double iwr = fmin(p[2], t[2]) - fmax(p[0], t[0]), ihr = fmin(p[3], t[3]) - fmax(p[1], t[1]);
    const double iw = fmax(iwr, 0.0), ih = fmax(ihr, 0.0);
    const double inter = iw * ih;
    const double uni = area1 + area2 - inter;
    const double U = uni + eps;
    const double iou = inter / U;
    // the loss as a function of (iou, uni, ew, eh, ddx, ddy, w1, h1): its partial derivatives
    double g_iou = -1.0, g_uni = 0.0, g_ew = 0.0, g_eh = 0.0, g_ddx = 0.0, g_ddy = 0.0, g_w1 = 0.0, g_h1 = 0.0;
    if (kind >= 3) {
        const double ew = fmax(p[2], t[2]) - fmin(p[0], t[0]), eh = fmax(p[3], t[3]) - fmin(p[1], t[1]);
        if (kind == 3) {
            const double enclosing = ew * eh;
            const double g_enc = uni / (enclosing * enclosing);
            g_uni = -1.0 / enclosing;
            g_ew = g_enc * eh; g_eh = g_enc * ew;
        } else {
            const double diagonal = ew * ew + eh * eh;
            const double ddx = (t[0] + t[2]) / 2.0 - (p[0] + p[2]) / 2.0, ddy = (t[1] + t[3]) / 2.0 - (p[1] + p[3]) / 2.0;
            const double g_diag = -(ddx * ddx + ddy * ddy) / (diagonal * diagonal);
            g_ew = g_diag * (2.0 * ew); g_eh = g_diag * (2.0 * eh);
            g_ddx = 2.0 * ddx / diagonal; g_ddy = 2.0 * ddy / diagonal;
            if (kind == 5) {
                const double w2 = t[2] - t[0], h2 = t[3] - t[1];
                const double hq = h1 + eps, q = w1 / hq;
                const double angle = (atan(q) - atan(w2 / (h2 + eps))) * 2.0 / 3.141592653589793;
                const double v = angle * angle;
                const double r = v / (1.0 - iou + v + eps);               // alpha; the term is r v
                g_iou = -1.0 + r * r;
                const double g_q = (2.0 * r - r * r) * (2.0 * angle) * (2.0 / 3.141592653589793) / (1.0 + q * q);
                g_w1 = g_q / hq; g_h1 = -(g_q * w1) / (hq * hq);
            }
        }
    }
    const double g_uni_t = g_uni - g_iou * (inter / (U * U));
    const double g_inter = g_iou / U - g_uni_t;
    const double g_iw = iwr >= 0.0 ? g_inter * ih : 0.0, g_ih = ihr >= 0.0 ? g_inter * iw : 0.0;      // clamp at 0: passes at >= 0
    const double ax = g_uni_t * h1, ay = g_uni_t * w1;        // through area1 = w1 h1
    g[0] = -(g_iw * d_max(p[0], t[0])) - ax - g_ew * d_min(p[0], t[0]) - 0.5 * g_ddx - g_w1;
    g[1] = -(g_ih * d_max(p[1], t[1])) - ay - g_eh * d_min(p[1], t[1]) - 0.5 * g_ddy - g_h1;
    g[2] = g_iw * d_min(p[2], t[2]) + ax + g_ew * d_max(p[2], t[2]) - 0.5 * g_ddx + g_w1;
    g[3] = g_ih * d_min(p[3], t[3]) + ay + g_eh * d_max(p[3], t[3]) - 0.5 * g_ddy + g_h1;
}

struct BoxGradArgs {
    const float* box; long sn, sc, sh, sw;
    float* grad; long gn, gc, gh, gw;
    const double* gt_boxes;
    const Rec* rec;
    const int* count;
    const double* counts;
    const double* scales;
    int H, W, Gmax, tx;
    int kind, box_log;
    float mult, stride;
};

__global__ __launch_bounds__(THREADS) void box_grad_kernel(const BoxGradArgs a) {
    __shared__ int4 s_smp[PASS_SLOTS];
    __shared__ int s_cnt[WAVES];
    const int tid = threadIdx.x;
    const Tile tile(blockIdx.x, a.tx, a.H, a.W);
    const int n = tile.n, x0 = tile.x0, y0 = tile.y0, x1 = tile.x1, y1 = tile.y1;
    const int x = x0 + tid % TILE_W, y = y0 + tid / TILE_W;
    const bool inside = tile.holds(x, y);
    const int M = min(max(a.count[n], 0), a.Gmax);
    const Rec* const recs = a.rec + (long)n * a.Gmax;
    const double* const gts = a.gt_boxes + (long)n * a.Gmax * 4;
    const float* const bp = a.box + (long)n * a.sn + (long)y * a.sh + (long)x * a.sw;
    const double scale = (a.scales ? a.scales[1] : 1.0) / fmax(1.0, a.counts[1]);
    const int passes = (M + PASS_SLOTS - 1) / PASS_SLOTS;

    double acc[4] = {0.0, 0.0, 0.0, 0.0}, chain[4] = {0.0, 0.0, 0.0, 0.0};
    float pred[4] = {0.f, 0.f, 0.f, 0.f};
    bool touched = false;
    for (int p = 0; p < passes; ++p) {                        // (uniform: M is the image's)
        // the counted records whose SAMPLE neighbourhood (cx-1..cx+1 x cy-1..cy+1 clipped to the map: a radius-0 box still has nine samples, a
        // centre on cx == W samples column W - 1) touches the tile, as (cx, cy, slot, 0)
        const int cnt = stage_pass(p * PASS_SLOTS, M, s_smp, s_cnt, [&](int s, int4& v) {
            const Rec r = recs[s];
            v = make_int4(r.cx, r.cy, s, 0);
            return r.state != 0 && max(r.cx - 1, 0) < x1 && min(r.cx + 1, a.W - 1) >= x0 && max(r.cy - 1, 0) < y1 && min(r.cy + 1, a.H - 1) >= y0;
        });
        if (!inside) continue;
        for (int j = 0; j < cnt; ++j) {
            const int4 r = s_smp[j];                          // the same address in every lane: a broadcast
            if (abs(x - r.x) > 1 || abs(y - r.y) > 1) continue;
            if (!touched) {                                   // this pixel's decode and its derivative, once
                touched = true;
                cnl::decode_box(bp, a.sc, x, y, a.W, a.H, 0, a.box_log, a.mult, a.stride, pred);
#pragma unroll
                for (int k = 0; k < 4; ++k) {                 // the decode's own fp32 operations (box_decode.h), for the clamp's side and exp's value
                    float v = bp[(long)k * a.sc];
                    if (a.box_log) v = expf(v);
                    const float m = v * a.mult;
                    const double side = k < 2 ? -1.0 : 1.0;   // x1 = (cx + 0.5 - g) stride, x2 = (cx + 0.5 + g) stride
                    chain[k] = m >= 0.f ? side * (double)a.stride * (double)a.mult * (a.box_log ? (double)v : 1.0) : 0.0;
                }
            }
            const double* const b = gts + (long)r.z * 4;
            const float target[4] = {(float)b[0], (float)b[1], (float)(b[0] + b[2]), (float)(b[1] + b[3])};
            double g[4];
            box_dterm(a.kind, pred, target, g);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += g[k] * chain[k];
        }
    }
    if (inside) {
        float* const o = a.grad + (long)n * a.gn + (long)y * a.gh + (long)x * a.gw;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[(long)k * a.gc] = touched ? (float)(scale * acc[k]) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct Call {                                      // what both entry points take
    const float* heat; int64_t sn, sc, sh, sw;
    const float* box;
    int N, C, H, W, Gmax;
    const double* gt_boxes; const int64_t* gt_labels; const int32_t* gt_count;
    const cnl_loss_params* p;
};

// the checks both entry points make before an empty batch returns
inline int check_call(const Call& c, const char* who) {
    const cnl_loss_params* const p = c.p;
    CNL_REQUIRE(p, CNL_E_BAD_ARG, "%s: null params", who);
    if (int rc = check_dims(who, c.N, c.H, c.W, c.Gmax)) return rc;
    CNL_REQUIRE(c.C >= 1 && c.C <= MAX_C, CNL_E_BAD_ARG, "%s: C = %d outside 1..2^16", who, c.C);
    CNL_REQUIRE(p->target_method >= 0 && p->target_method <= 2, CNL_E_BAD_ARG, "%s: target_method = %d outside 0..2", who, p->target_method);
    CNL_REQUIRE(p->heatmap_loss >= 0 && p->heatmap_loss <= 1, CNL_E_BAD_ARG, "%s: heatmap_loss = %d outside 0..1", who, p->heatmap_loss);
    CNL_REQUIRE(p->box_loss >= 0 && p->box_loss <= 5, CNL_E_BAD_ARG, "%s: box_loss = %d outside 0..5", who, p->box_loss);
    if (int rc = check_stride(who, p->stride)) return rc;
    CNL_REQUIRE(p->target_method != 0 || (p->target_param > 0.0 && p->target_param < 1.0), CNL_E_BAD_ARG, "%s: cornernet min_overlap = %g outside (0, 1)",
                who, p->target_param);
    CNL_REQUIRE(p->target_param == p->target_param && p->hm_alpha == p->hm_alpha && p->hm_beta == p->hm_beta, CNL_E_BAD_ARG, "%s: a NaN parameter", who);
    return CNL_OK;
}

inline int launch_records(const Call& c, Rec* rec, hipStream_t st) {
    const long slots = (long)c.N * c.Gmax;
    hipLaunchKernelGGL(record_kernel, dim3((unsigned)((slots + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, c.gt_boxes,
                       reinterpret_cast<const long long*>(c.gt_labels), c.gt_count, c.N, c.Gmax, c.C, c.H, c.W, c.p->stride, c.p->target_method,
                       c.p->target_param, rec);
    return cnl::check_launch("det_loss record_kernel");
}

inline void fill(HeatArgs& a, const Call& c, const Rec* rec) {
    const cnl_loss_params* const p = c.p;
    a.heat = c.heat; a.sn = c.sn; a.sc = c.sc; a.sh = c.sh; a.sw = c.sw;
    a.rec = rec; a.count = c.gt_count; a.part = nullptr; a.counts = a.scales = nullptr;
    a.C = c.C; a.H = c.H; a.W = c.W; a.Gmax = c.Gmax; a.tx = tiles_x(c.W);
    a.loss = p->heatmap_loss; a.alpha = p->hm_alpha; a.beta = p->hm_beta;
    a.alpha_is_2 = p->hm_alpha == 2.0; a.beta_is_4 = p->hm_beta == 4.0; a.beta_is_2 = p->hm_beta == 2.0;
}

}  // namespace cnl_det_loss

extern "C" size_t cnl_detection_loss_workspace_bytes(int32_t N, int32_t Gmax, int32_t H, int32_t W) {
    using namespace cnl_det_loss;
    return dims_in_range(N, Gmax, H, W) ? sections(N, Gmax, H, W).total : 0;
}

extern "C" int cnl_detection_loss_f64(const float* heat, int64_t heat_sn, int64_t heat_sc, int64_t heat_sh, int64_t heat_sw, const float* box,
                                      int64_t box_sn, int64_t box_sc, int64_t box_sh, int64_t box_sw, int32_t N, int32_t C, int32_t H, int32_t W,
                                      const double* gt_boxes, const int64_t* gt_labels, const int32_t* gt_count, int32_t Gmax,
                                      const cnl_loss_params* p, float* target_map, int64_t t_sn, int64_t t_sc, int64_t t_sh, int64_t t_sw,
                                      double* per_image, double* totals, int32_t* skipped, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace cnl_det_loss;
    const char* const who = "cnl_detection_loss_f64";
    const Call c{heat, heat_sn, heat_sc, heat_sh, heat_sw, box, N, C, H, W, Gmax, gt_boxes, gt_labels, gt_count, p};
    if (int rc = check_call(c, who)) return rc;
    CNL_REQUIRE((heat != nullptr) == (box != nullptr), CNL_E_BAD_ARG, "%s: heat and box come together (both NULL: targets only)", who);
    CNL_REQUIRE(heat || target_map, CNL_E_BAD_ARG, "%s: neither logits nor a target map: nothing to do", who);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(gt_boxes && gt_labels && gt_count && per_image && totals && skipped && workspace, CNL_E_BAD_ARG, "%s: null pointer", who);
    if (int rc = check_aligned(who, {gt_boxes, gt_labels, per_image, totals}, workspace, {heat, box, target_map, gt_count, skipped})) return rc;
    const Sections sec = sections(N, Gmax, H, W);
    if (int rc = check_workspace(who, workspace_bytes, sec.total)) return rc;
    int tiles;
    if (int rc = check_tile_grid(who, N, H, W, tiles)) return rc;
    char* const ws = static_cast<char*>(workspace);
    Rec* const rec = reinterpret_cast<Rec*>(ws + sec.rec);
    double* const part = reinterpret_cast<double*>(ws + sec.part);
    double* const img = reinterpret_cast<double*>(ws + sec.img);
    hipStream_t st = (hipStream_t)stream;

    if (int rc = launch_records(c, rec, st)) return rc;

    HeatArgs a;
    fill(a, c, rec);
    a.out = target_map; a.on = t_sn; a.oc = t_sc; a.oh = t_sh; a.ow = t_sw;
    a.part = part;
    const dim3 grid((unsigned)(N * tiles));
    // with logits their layout picks the element order; a targets-only launch follows the target map's
    const int64_t l_sc = heat ? heat_sc : t_sc, l_sw = heat ? heat_sw : t_sw;
    if (l_sc == 1) hipLaunchKernelGGL(heatmap_kernel<LAYOUT_CMINOR>, grid, dim3(THREADS), 0, st, a);
    else if (l_sw == 1 && heat) hipLaunchKernelGGL(heatmap_kernel<LAYOUT_PLANE>, grid, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL(heatmap_kernel<LAYOUT_GENERIC>, grid, dim3(THREADS), 0, st, a);
    if (int rc = cnl::check_launch("det_loss heatmap_kernel")) return rc;

    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)N), dim3(THREADS), 0, st, box, (long)box_sn, (long)box_sc, (long)box_sh, (long)box_sw, gt_boxes,
                       gt_count, rec, Gmax, H, W, p->box_loss, p->box_log, p->box_multiplier, (float)p->stride, img);
    if (int rc = cnl::check_launch("det_loss sample_kernel")) return rc;

    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(THREADS), 0, st, part, img, N, tiles, p->heatmap_weight, p->box_weight, per_image, totals, skipped);
    return cnl::check_launch("det_loss finish_kernel");
}

extern "C" size_t cnl_detection_loss_grad_workspace_bytes(int32_t N, int32_t Gmax, int32_t H, int32_t W) {
    using namespace cnl_det_loss;
    return dims_in_range(N, Gmax, H, W) ? grad_sections_total(N, Gmax) : 0;
}

extern "C" int cnl_detection_loss_grad_f32(const float* heat, int64_t heat_sn, int64_t heat_sc, int64_t heat_sh, int64_t heat_sw, const float* box,
                                           int64_t box_sn, int64_t box_sc, int64_t box_sh, int64_t box_sw, int32_t N, int32_t C, int32_t H, int32_t W,
                                           const double* gt_boxes, const int64_t* gt_labels, const int32_t* gt_count, int32_t Gmax,
                                           const cnl_loss_params* p, const double* scales, float* grad_heat, int64_t gh_sn, int64_t gh_sc,
                                           int64_t gh_sh, int64_t gh_sw, float* grad_box, int64_t gb_sn, int64_t gb_sc, int64_t gb_sh, int64_t gb_sw,
                                           int32_t* skipped, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace cnl_det_loss;
    const char* const who = "cnl_detection_loss_grad_f32";
    const Call c{heat, heat_sn, heat_sc, heat_sh, heat_sw, box, N, C, H, W, Gmax, gt_boxes, gt_labels, gt_count, p};
    if (int rc = check_call(c, who)) return rc;
    CNL_REQUIRE(heat && box, CNL_E_BAD_ARG, "%s: the gradient needs the logits and the box map", who);
    if (N == 0) return CNL_OK;
    CNL_REQUIRE(gt_boxes && gt_labels && gt_count && skipped && workspace, CNL_E_BAD_ARG, "%s: null pointer", who);
    if (int rc = check_aligned(who, {gt_boxes, gt_labels, scales}, workspace, {heat, box, grad_heat, grad_box, gt_count, skipped})) return rc;
    if (int rc = check_workspace(who, workspace_bytes, grad_sections_total(N, Gmax))) return rc;
    int tiles;
    if (int rc = check_tile_grid(who, N, H, W, tiles)) return rc;
    char* const ws = static_cast<char*>(workspace);
    Rec* const rec = reinterpret_cast<Rec*>(ws);
    double* const counts = reinterpret_cast<double*>(ws + (size_t)N * Gmax * sizeof(Rec));
    hipStream_t st = (hipStream_t)stream;

    if (int rc = launch_records(c, rec, st)) return rc;
    hipLaunchKernelGGL(count_kernel, dim3(1), dim3(THREADS), 0, st, rec, gt_count, N, Gmax, H, W, counts, skipped);
    if (int rc = cnl::check_launch("det_loss count_kernel")) return rc;
    const dim3 grid((unsigned)(N * tiles));

    if (grad_heat) {
        HeatArgs a;
        fill(a, c, rec);
        a.out = grad_heat; a.on = gh_sn; a.oc = gh_sc; a.oh = gh_sh; a.ow = gh_sw;
        a.counts = counts; a.scales = scales;
        // the element order follows the gradient's strides; four elements per lane where both maps are packed channels-last rows of whole 16-byte groups
        auto packed = [&](const float* ptr, int64_t sn, int64_t sc, int64_t sh, int64_t sw) {
            return sc == 1 && sw == C && sh % 4 == 0 && sn % 4 == 0 && ((uintptr_t)ptr & 15) == 0;
        };
        const bool vec4 = ((long long)W * C) % 4 == 0 && packed(heat, heat_sn, heat_sc, heat_sh, heat_sw) && packed(grad_heat, gh_sn, gh_sc, gh_sh, gh_sw);
        if (vec4) hipLaunchKernelGGL((heat_grad_kernel<LAYOUT_CMINOR, true>), grid, dim3(THREADS), 0, st, a);
        else if (gh_sc == 1) hipLaunchKernelGGL((heat_grad_kernel<LAYOUT_CMINOR, false>), grid, dim3(THREADS), 0, st, a);
        else if (gh_sw == 1) hipLaunchKernelGGL((heat_grad_kernel<LAYOUT_PLANE, false>), grid, dim3(THREADS), 0, st, a);
        else hipLaunchKernelGGL((heat_grad_kernel<LAYOUT_GENERIC, false>), grid, dim3(THREADS), 0, st, a);
        if (int rc = cnl::check_launch("det_loss heat_grad_kernel")) return rc;
    }
    if (grad_box) {
        BoxGradArgs b;
        b.box = box; b.sn = box_sn; b.sc = box_sc; b.sh = box_sh; b.sw = box_sw;
        b.grad = grad_box; b.gn = gb_sn; b.gc = gb_sc; b.gh = gb_sh; b.gw = gb_sw;
        b.gt_boxes = gt_boxes; b.rec = rec; b.count = gt_count; b.counts = counts; b.scales = scales;
        b.H = H; b.W = W; b.Gmax = Gmax; b.tx = tiles_x(W);
        b.kind = p->box_loss; b.box_log = p->box_log; b.mult = p->box_multiplier; b.stride = (float)p->stride;
        hipLaunchKernelGGL(box_grad_kernel, grid, dim3(THREADS), 0, st, b);
        if (int rc = cnl::check_launch("det_loss box_grad_kernel")) return rc;
    }
    return CNL_OK;
}
