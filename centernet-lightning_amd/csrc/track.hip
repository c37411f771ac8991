// track.hip — the tracker's association costs and track-table update, so that the k x 64
// embeddings of every frame stay in HBM: only the small n x T cost matrices travel to the host for the Hungarian step
// (scipy, as in the reference) and the match list travels back.
//
// Replaces, per frame, of centernet_lightning/models/tracker.py:
//   :133-137  detection-threshold mask + boolean-mask compaction of bboxes / labels / embeddings
//   :150      reid_cost = scipy cdist(det_embeddings, track_embeddings, "cosine")                 -> float64 [n, T]
//   :162      box_cost  = box_iou_distance_matrix | box_giou_distance_matrix (utils/box.py:49-92) -> float32 [n, T]
//   :228,320-321  Track.embedding = e/|e| ; (1-s)*old + s*e/|e|  and  Track.bbox = bbox (use_kalman=False)
//
// Arithmetic mirrors the CPU libraries operation by operation (no fma contraction) so that the integer decisions taken
// from the costs (thresholds, Hungarian assignment) are the reference's: the cosine distance is evaluated in float64 with the
// sequential dot product, the |cos| <= 1 clamp and 1 - cos of scipy's cdist; the box distances in float32 in numpy's order.
// cnl_track_frame_gated_f32 (frame_gated_kernel) writes the same record with the class / motion gates of cnl_track_gate applied inside the
// per-pair cost functions (track_costs.h): no counterpart in the reference, whose tracker.py:145-147 leaves class filtering as a TODO.
#include "track_costs.h"      // compact_scores / pair_costs (shared with track_streams.hip)

#pragma clang fp contract(off)   // one rounding per operation, like numpy / scipy: the costs feed thresholds and the Hungarian step

namespace cnl_track {

// Every workgroup handles 256 (detection, track) pairs; workgroup 0 also publishes n_det / det_index.
__global__ __launch_bounds__(256) void costs_kernel(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                    const float* __restrict__ det_score, int k, int E, float thr,
                                                    const float* __restrict__ trk_emb, const float* __restrict__ trk_box, int T,
                                                    int box_mode, int reid_metric, int* __restrict__ n_det, int* __restrict__ det_index,
                                                    double* __restrict__ reid_cost, float* __restrict__ box_cost) {
    __shared__ int sel[MAXK];
    __shared__ int wave_sum[4];
    const int n = compact_scores(det_score, k, thr, sel, wave_sum);
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *n_det = n;
        for (int i = threadIdx.x; i < n; i += 256) det_index[i] = sel[i];
    }
    pair_costs(sel, n, det_emb, det_box, E, trk_emb, trk_box, T, box_mode, reid_metric, reid_cost, box_cost);
}

// The same, writing ONE self-describing record (include/centernet_gfx950.h: cnl_track_frame_f32) whose cost matrices are packed by the
// n the kernel itself found — so the host needs no copy of the scores before the launch, and the record may live in page-locked host
// memory mapped into the device's address space: the frame's only device -> host traffic is these stores, no copy engine involved.
// LOW (cnl_track_frame_low_f32): a 48-byte header, and behind the box matrix the low-score detections {i : low_thr <= score[i] < thr} and their
// box costs, for the host's third association stage.
// GATED (cnl_track_frame_gated_f32): the class / motion gates inside the per-pair cost functions; every other byte as LOW writes it.
template <bool LOW, bool GATED>
__device__ __forceinline__ void frame_body(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                           const float* __restrict__ det_score, const void* __restrict__ det_label, int label_kind,
                                           int k, int E, float thr, float low_thr, const float* __restrict__ trk_emb,
                                           const float* __restrict__ trk_box, int T, int box_mode, int reid_metric, int with_dets,
                                           char* __restrict__ record, const GateOps& g) {
    __shared__ int sel[MAXK];
    __shared__ int low_sel[LOW ? MAXK : 1];
    __shared__ int wave_sum[4];
    const int n = compact_scores(det_score, k, thr, sel, wave_sum);
    const int n_low = LOW ? compact_scores_in<true>(det_score, k, low_thr, thr, low_sel, wave_sum) : 0;
    const int off_index = LOW ? 48 : 32, off_dets = (off_index + 4 * k + 7) & ~7, off_reid = (off_dets + (with_dets ? 24 * k : 0) + 7) & ~7;
    const long off_box = off_reid + 8l * n * T, off_low_index = off_box + 4l * n * T, off_low_box = off_low_index + 4l * k;
    if (blockIdx.x == 0) {
        const int tid = threadIdx.x;
        int* hdr = reinterpret_cast<int*>(record);
        if (tid == 0) { hdr[0] = n; hdr[1] = k; hdr[2] = T; hdr[3] = with_dets; hdr[4] = off_index; hdr[5] = off_dets; hdr[6] = off_reid; hdr[7] = (int)off_box; }
        if (LOW) {
            if (tid == 0) { hdr[8] = n_low; hdr[9] = (int)off_low_index; hdr[10] = (int)off_low_box; hdr[11] = 0; }
            int* low_index = reinterpret_cast<int*>(record + off_low_index);
            for (int i = tid; i < n_low; i += 256) low_index[i] = low_sel[i];
        }
        int* det_index = reinterpret_cast<int*>(record + off_index);
        for (int i = tid; i < n; i += 256) det_index[i] = sel[i];
        if (with_dets) {      // the frame's boxes / scores / labels, which the host-side life cycle reads (tracker.py:171-186)
            float* o = reinterpret_cast<float*>(record + off_dets);
            for (int i = tid; i < 4 * k; i += 256) o[i] = det_box[i];
            for (int i = tid; i < k; i += 256) o[4 * k + i] = det_score[i];
            int* ol = reinterpret_cast<int*>(o + 5 * k);
            for (int i = tid; i < k; i += 256)
                ol[i] = label_kind == 1 ? (int)reinterpret_cast<const long long*>(det_label)[i]
                      : label_kind == 2 ? reinterpret_cast<const int*>(det_label)[i]
                      : label_kind == 3 ? (int)reinterpret_cast<const float*>(det_label)[i] : 0;
        }
    }
    pair_costs_at<GATED>((long)blockIdx.x * 256 + threadIdx.x, sel, n, det_emb, det_box, E, trk_emb, trk_box, T, box_mode, reid_metric,
                         reinterpret_cast<double*>(record + off_reid), reinterpret_cast<float*>(record + off_box), g);
    if (LOW)      // n_low <= k: the grid that covers k * T pairs covers these
        pair_box_cost_at<GATED>((long)blockIdx.x * 256 + threadIdx.x, low_sel, n_low, det_box, trk_box, T, box_mode,
                                reinterpret_cast<float*>(record + off_low_box), g);
}

template <bool LOW>
__global__ __launch_bounds__(256) void frame_kernel(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                    const float* __restrict__ det_score, const void* __restrict__ det_label, int label_kind,
                                                    int k, int E, float thr, float low_thr, const float* __restrict__ trk_emb,
                                                    const float* __restrict__ trk_box, int T, int box_mode, int reid_metric, int with_dets,
                                                    char* __restrict__ record) {
    frame_body<LOW, false>(det_emb, det_box, det_score, det_label, label_kind, k, E, thr, low_thr, trk_emb, trk_box, T, box_mode, reid_metric, with_dets,
                           record, GateOps{});
}

__global__ __launch_bounds__(256) void frame_gated_kernel(const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                          const float* __restrict__ det_score, const void* __restrict__ det_label, int label_kind,
                                                          int k, int E, float thr, float low_thr, const float* __restrict__ trk_emb,
                                                          const float* __restrict__ trk_box, int T, int box_mode, int reid_metric, int with_dets,
                                                          char* __restrict__ record, GateOps g) {
    frame_body<true, true>(det_emb, det_box, det_score, det_label, label_kind, k, E, thr, low_thr, trk_emb, trk_box, T, box_mode, reid_metric, with_dets, record,
                           g);
}

// One wave per row of the new track table.  KEEP (cnl_track_apply_keep_f32): a matched row whose keep_emb byte is set takes the detection's
// box and the old row's embedding.
template <bool KEEP>
__global__ __launch_bounds__(64) void apply_kernel(const float* __restrict__ trk_emb, const float* __restrict__ trk_box,
                                                   const float* __restrict__ det_emb, const float* __restrict__ det_box,
                                                   const int* __restrict__ src_trk, const int* __restrict__ src_det,
                                                   const uint8_t* __restrict__ keep_emb, int E, float keep, float blend,
                                                   float* __restrict__ new_emb, float* __restrict__ new_box) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int t = src_trk[r], d = src_det[r];
    const bool carry = d < 0 || (KEEP && t >= 0 && keep_emb[r] != 0);      // the embedding is the old row's
    float inv_den = 0.f;
    if (!carry) {      // |e| = sqrt(sum e^2) in float32 (np.linalg.norm of a float32 vector)
        float s = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float x = det_emb[(long)d * E + e];
            s += x * x;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        inv_den = sqrtf(s);
    }
    for (int e = lane; e < E; e += 64) {
        float v;
        if (carry) v = trk_emb[(long)t * E + e];
        else {
            const float unit = (det_emb[(long)d * E + e] / inv_den);
            v = t < 0 ? unit : ((keep * trk_emb[(long)t * E + e]) + (blend * unit));
        }
        new_emb[(long)r * E + e] = v;
    }
    if (lane < 4) new_box[(long)r * 4 + lane] = d >= 0 ? det_box[(long)d * 4 + lane] : trk_box[(long)t * 4 + lane];
}

}  // namespace cnl_track
using namespace cnl_track;

extern "C" int cnl_track_costs_metric_f32(const float* det_emb, const float* det_box, const float* det_score, int32_t k, int32_t E,
                                          float detection_threshold, const float* trk_emb, const float* trk_box, int32_t T,
                                          int32_t box_cost, int32_t reid_metric, int32_t* n_det, int32_t* det_index, double* reid_cost,
                                          float* box_cost_out, void* stream) {
    CNL_REQUIRE(det_emb && det_box && det_score && n_det && det_index, CNL_E_BAD_ARG, "cnl_track_costs_f32: null pointer");
    CNL_REQUIRE(k > 0 && E > 0 && T >= 0, CNL_E_BAD_ARG, "cnl_track_costs_f32: bad k/E/T");
    CNL_REQUIRE(k <= MAXK, CNL_E_UNSUPPORTED, "cnl_track_costs_f32: k = %d > %d detections per frame", k, MAXK);
    CNL_REQUIRE(box_cost >= 0 && box_cost <= 2, CNL_E_BAD_ARG, "cnl_track_costs_f32: box_cost must be 0 (none), 1 (iou), 2 (giou)");
    CNL_REQUIRE(reid_metric >= 0 && reid_metric <= 7, CNL_E_BAD_ARG, "cnl_track_costs_metric_f32: reid_metric must be 0 (cosine), 1 (euclidean), 2 (sqeuclidean), 3 (cityblock), 4 (chebyshev), 5 (canberra), 6 (braycurtis) or 7 (correlation)");
    CNL_REQUIRE(T == 0 || (trk_emb && reid_cost), CNL_E_BAD_ARG, "cnl_track_costs_f32: T > 0 without track table / reid_cost");
    CNL_REQUIRE(T == 0 || box_cost == 0 || (trk_box && box_cost_out), CNL_E_BAD_ARG,
                "cnl_track_costs_f32: box cost requested without track boxes / output");
    CNL_REQUIRE(inputs_aligned(det_emb, det_box, trk_emb, trk_box, E, T, box_cost), CNL_E_BAD_ARG, "cnl_track_costs_metric_f32: %s", INPUTS_ALIGNED);
    const long pairs = (long)k * T;
    const unsigned grid = (unsigned)(pairs > 0 ? (pairs + 255) / 256 : 1);
    hipLaunchKernelGGL(costs_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, det_emb, det_box, det_score, k, E,
                       detection_threshold, trk_emb, trk_box, T, box_cost, reid_metric, n_det, det_index, reid_cost, box_cost_out);
    return cnl::check_launch("track costs_kernel");
}

// bytes of a frame record: [header | det_index[k] | (detections) | reid | box] and, LOW, [low_index[k] | low_box] behind them.  The worst case
// is n = k; the kept and the low detections are disjoint (n + n_low <= k), so 12 k T bounds 12 n T + 4 n_low T as well.
static int64_t frame_bytes(int32_t k, int32_t T, int32_t with_detections, bool low) {
    if (k <= 0 || T < 0) return 0;
    const int64_t off_dets = ((low ? 48 : 32) + 4l * k + 7) & ~7l, off_reid = (off_dets + (with_detections ? 24l * k : 0) + 7) & ~7l;
    return off_reid + 12l * k * T + (low ? 4l * k : 0);
}
extern "C" int64_t cnl_track_frame_bytes(int32_t k, int32_t T, int32_t with_detections) { return frame_bytes(k, T, with_detections, false); }
extern "C" int64_t cnl_track_frame_low_bytes(int32_t k, int32_t T, int32_t with_detections) { return frame_bytes(k, T, with_detections, true); }

// cnl_track_frame_f32 (low = false; low_threshold unused), cnl_track_frame_low_f32 and cnl_track_frame_gated_f32 (low, gate set; without a low-score
// stage — low_threshold == detection_threshold, n_low = 0 — it also takes box_cost 0): one set of checks, one kernel body.
static int frame_launch(const char* name, bool low, const cnl_track_gate* gate, const float* det_emb, const float* det_box, const float* det_score, const void* det_label,
                        int32_t label_kind, int32_t k, int32_t E, float detection_threshold, float low_threshold, const float* trk_emb,
                        const float* trk_box, int32_t T, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record,
                        int64_t record_bytes, void* stream) {
    CNL_REQUIRE(det_emb && det_box && det_score && record, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(k > 0 && E > 0 && T >= 0, CNL_E_BAD_ARG, "%s: bad k/E/T", name);
    CNL_REQUIRE(k <= MAXK, CNL_E_UNSUPPORTED, "%s: k = %d > %d detections per frame", name, k, MAXK);
    const bool low_stage = low && !(gate != nullptr && low_threshold == detection_threshold);
    CNL_REQUIRE(box_cost >= (low_stage ? 1 : 0) && box_cost <= 2, CNL_E_BAD_ARG, "%s: box_cost must be %s1 (iou), 2 (giou)", name, low_stage ? "" : "0 (none), ");
    CNL_REQUIRE(!low || (low_threshold >= 0.f && low_threshold <= detection_threshold), CNL_E_BAD_ARG,
                "%s: low_threshold %g must lie in [0, detection_threshold = %g]", name, (double)low_threshold, (double)detection_threshold);
    CNL_REQUIRE(reid_metric >= 0 && reid_metric <= 7, CNL_E_BAD_ARG, "%s: reid_metric must be 0 (cosine) .. 7 (correlation)", name);
    CNL_REQUIRE(label_kind >= 0 && label_kind <= 3 && (label_kind == 0 || det_label), CNL_E_BAD_ARG,
                "%s: label_kind must be 0 (none), 1 (int64), 2 (int32), 3 (float32) with det_label set", name);
    if (int rc = check_gate(name, gate, det_box, {})) return rc;
    CNL_REQUIRE(T == 0 || trk_emb, CNL_E_BAD_ARG, "%s: T > 0 without track table", name);
    CNL_REQUIRE(T == 0 || box_cost == 0 || trk_box, CNL_E_BAD_ARG, "%s: box cost requested without track boxes", name);
    CNL_REQUIRE(((uintptr_t)record & 7) == 0, CNL_E_BAD_ARG, "%s: record must be 8-byte aligned", name);
    CNL_REQUIRE(inputs_aligned(det_emb, det_box, trk_emb, trk_box, E, T, box_cost), CNL_E_BAD_ARG, "%s: %s", name, INPUTS_ALIGNED);
    const int64_t need = frame_bytes(k, T, with_detections, low);
    CNL_REQUIRE(record_bytes >= need && need < (1l << 31), record_bytes < need ? CNL_E_BAD_ARG : CNL_E_UNSUPPORTED,
                "%s: record holds %ld bytes, k = %d, T = %d needs %ld (cnl_track_frame%s_bytes; below 2 GiB)", name, (long)record_bytes, k, T, (long)need,
                low ? "_low" : "");
    const long pairs = (long)k * T;
    const unsigned grid = (unsigned)(pairs > 0 ? (pairs + 255) / 256 : 1);
    if (gate != nullptr) {
        const GateOps g{gate->trk_label, gate->kx, gate->kP, gate->motion_gate, gate->motion_weight, det_label, label_kind, 0};
        hipLaunchKernelGGL(frame_gated_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, det_emb, det_box, det_score, det_label, label_kind, k, E,
                           detection_threshold, low_threshold, trk_emb, trk_box, T, box_cost, reid_metric, with_detections ? 1 : 0, (char*)record, g);
        return cnl::check_launch("track frame_gated_kernel");
    }
    hipLaunchKernelGGL(low ? frame_kernel<true> : frame_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, det_emb, det_box, det_score, det_label,
                       label_kind, k, E, detection_threshold, low_threshold, trk_emb, trk_box, T, box_cost, reid_metric, with_detections ? 1 : 0,
                       (char*)record);
    return cnl::check_launch("track frame_kernel");
}

extern "C" int cnl_track_frame_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                   int32_t k, int32_t E, float detection_threshold, const float* trk_emb, const float* trk_box, int32_t T,
                                   int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record, int64_t record_bytes,
                                   void* stream) {
    return frame_launch("cnl_track_frame_f32", false, nullptr, det_emb, det_box, det_score, det_label, label_kind, k, E, detection_threshold, 0.f, trk_emb, trk_box,
                        T, box_cost, reid_metric, with_detections, record, record_bytes, stream);
}

extern "C" int cnl_track_frame_low_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                       int32_t k, int32_t E, float detection_threshold, float low_threshold, const float* trk_emb,
                                       const float* trk_box, int32_t T, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record,
                                       int64_t record_bytes, void* stream) {
    return frame_launch("cnl_track_frame_low_f32", true, nullptr, det_emb, det_box, det_score, det_label, label_kind, k, E, detection_threshold, low_threshold,
                        trk_emb, trk_box, T, box_cost, reid_metric, with_detections, record, record_bytes, stream);
}

extern "C" int cnl_track_frame_gated_f32(const float* det_emb, const float* det_box, const float* det_score, const void* det_label, int32_t label_kind,
                                         int32_t k, int32_t E, float detection_threshold, float low_threshold, const float* trk_emb,
                                         const float* trk_box, int32_t T, int32_t box_cost, int32_t reid_metric, int32_t with_detections, void* record,
                                         int64_t record_bytes, const cnl_track_gate* gate, void* stream) {
    static const cnl_track_gate off = {nullptr, nullptr, nullptr, 0.0, 1.0};
    return frame_launch("cnl_track_frame_gated_f32", true, gate ? gate : &off, det_emb, det_box, det_score, det_label, label_kind, k, E, detection_threshold,
                        low_threshold, trk_emb, trk_box, T, box_cost, reid_metric, with_detections, record, record_bytes, stream);
}

extern "C" int cnl_track_costs_f32(const float* det_emb, const float* det_box, const float* det_score, int32_t k, int32_t E,
                                   float detection_threshold, const float* trk_emb, const float* trk_box, int32_t T,
                                   int32_t box_cost, int32_t* n_det, int32_t* det_index, double* reid_cost,
                                   float* box_cost_out, void* stream) {
    return cnl_track_costs_metric_f32(det_emb, det_box, det_score, k, E, detection_threshold, trk_emb, trk_box, T, box_cost, 0, n_det, det_index,
                                      reid_cost, box_cost_out, stream);
}

// cnl_track_apply_f32 (keep_emb null) and cnl_track_apply_keep_f32
static int apply_launch(const char* name, const float* trk_emb, const float* trk_box, const float* det_emb, const float* det_box,
                        const int32_t* src_trk, const int32_t* src_det, const uint8_t* keep_emb, int32_t T_new, int32_t E, double smoothing,
                        float* new_emb, float* new_box, void* stream) {
    CNL_REQUIRE(T_new >= 0 && E > 0, CNL_E_BAD_ARG, "%s: bad T_new/E", name);
    if (T_new == 0) return CNL_OK;
    CNL_REQUIRE(det_emb && det_box && src_trk && src_det && new_emb && new_box, CNL_E_BAD_ARG, "%s: null pointer", name);
    CNL_REQUIRE(new_emb != trk_emb && new_box != trk_box, CNL_E_BAD_ARG, "%s: the new table must not alias the old one", name);
    // tracker.py:321: (1 - s) and s are Python floats that numpy applies to float32 arrays as float32 scalars
    const float keep = (float)(1.0 - smoothing), blend = (float)smoothing;
    hipLaunchKernelGGL(keep_emb ? apply_kernel<true> : apply_kernel<false>, dim3((unsigned)T_new), dim3(64), 0, (hipStream_t)stream, trk_emb, trk_box,
                       det_emb, det_box, src_trk, src_det, keep_emb, E, keep, blend, new_emb, new_box);
    return cnl::check_launch("track apply_kernel");
}

extern "C" int cnl_track_apply_f32(const float* trk_emb, const float* trk_box, const float* det_emb, const float* det_box,
                                   const int32_t* src_trk, const int32_t* src_det, int32_t T_new, int32_t E, double smoothing,
                                   float* new_emb, float* new_box, void* stream) {
    return apply_launch("cnl_track_apply_f32", trk_emb, trk_box, det_emb, det_box, src_trk, src_det, nullptr, T_new, E, smoothing, new_emb, new_box, stream);
}

extern "C" int cnl_track_apply_keep_f32(const float* trk_emb, const float* trk_box, const float* det_emb, const float* det_box,
                                        const int32_t* src_trk, const int32_t* src_det, int32_t T_new, int32_t E, double smoothing,
                                        float* new_emb, float* new_box, const uint8_t* keep_emb, void* stream) {
    return apply_launch("cnl_track_apply_keep_f32", trk_emb, trk_box, det_emb, det_box, src_trk, src_det, keep_emb, T_new, E, smoothing, new_emb, new_box,
                        stream);
}
