"""ctypes binding of libcenternet_gfx950.so (C ABI: include/centernet_gfx950.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, the product path
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_void_p)

_LIB_NAME = "libcenternet_gfx950.so"
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", _LIB_NAME)

CNL_RELU = 1 << 0
CNL_SIGMOID = 1 << 1
CNL_UPSAMPLE_IN = 1 << 2
CNL_UPSAMPLE_OUT_ADD = 1 << 3
CNL_RELU6 = 1 << 4
CNL_W_SPLIT = 1 << 5          # cnl_conv_params.w is a cnl_conv_split_weights_f32 buffer (fp32 weights + their fp16 split)

# cnl_conv_params.algo: the arithmetic class a launch may use (include/centernet_gfx950.h)
CNL_ALGO_AUTO, CNL_ALGO_F2, CNL_ALGO_F32, CNL_ALGO_LATENCY, CNL_ALGO_F43, CNL_ALGO_FORCE = 0, 1, 2, 4, 5, 100
CNL_WINO_F32, CNL_WINO_F16X2 = 2, 5

CNL_E_BAD_ARG, CNL_E_UNSUPPORTED, CNL_E_WORKSPACE, CNL_E_HIP = -1, -2, -3, -4
ABI_VERSION = 13         # CNL_ABI_VERSION of include/centernet_gfx950.h


class ConvParams(Structure):
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("residual", c_void_p), ("y", c_void_p),
                ("N", c_int32), ("H_in", c_int32), ("W_in", c_int32), ("Cin", c_int32), ("Cout", c_int32),
                ("KH", c_int32), ("KW", c_int32), ("stride", c_int32), ("pad", c_int32),
                ("ldx", c_int32), ("ldy", c_int32), ("ldr", c_int32), ("flags", c_uint32),
                ("x_absmax", c_void_p), ("y_absmax", c_void_p), ("w_absmax", c_void_p), ("algo", c_uint32),
                ("splitk", c_int32), ("splitk_scratch", c_void_p), ("splitk_scratch_bytes", c_size_t),
                ("fuse_w", c_void_p), ("fuse_part", c_void_p), ("w_up", c_void_p)]


class DeconvParams(Structure):
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("residual", c_void_p), ("y", c_void_p),
                ("N", c_int32), ("H_in", c_int32), ("W_in", c_int32), ("Cin", c_int32), ("Cout", c_int32), ("K", c_int32),
                ("ldx", c_int32), ("ldy", c_int32), ("ldr", c_int32), ("flags", c_uint32)]


class DecodeParams(Structure):
    _fields_ = [("heat", c_void_p), ("heat_sn", c_int64), ("heat_sc", c_int64), ("heat_sh", c_int64), ("heat_sw", c_int64),
                ("box", c_void_p), ("box_sn", c_int64), ("box_sc", c_int64), ("box_sh", c_int64), ("box_sw", c_int64),
                ("reid", c_void_p), ("reid_sn", c_int64), ("reid_sc", c_int64), ("reid_sh", c_int64), ("reid_sw", c_int64),
                ("N", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32), ("E", c_int32),
                ("k", c_int32), ("nms_kernel", c_int32), ("normalize_boxes", c_int32), ("box_log", c_int32),
                ("box_multiplier", c_float), ("stride", c_float),
                ("scores", c_void_p), ("indices", c_void_p), ("labels", c_void_p), ("boxes", c_void_p), ("emb", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t)]


class LetterboxFrame(Structure):
    """cnl_letterbox_frame: one record of the table cnl_letterbox_bilinear_u8 / cnl_unletterbox_boxes_f32 read (40 bytes)."""
    _fields_ = [("src", c_void_p), ("h", c_int32), ("w", c_int32), ("row_stride", c_int32), ("new_h", c_int32), ("new_w", c_int32),
                ("pad_top", c_int32), ("pad_left", c_int32), ("reserved", c_int32)]


class Yuv420Frame(Structure):
    """cnl_yuv420_frame: one record of the table cnl_letterbox_yuv420_u8 reads (72 bytes)."""
    _fields_ = [("y", c_void_p), ("u", c_void_p), ("v", c_void_p), ("y_pitch", c_int32), ("c_pitch", c_int32), ("c_step", c_int32),
                ("x0", c_int32), ("y0", c_int32), ("h", c_int32), ("w", c_int32), ("new_h", c_int32), ("new_w", c_int32),
                ("pad_top", c_int32), ("pad_left", c_int32), ("reserved", c_int32)]


class MergeView(Structure):
    """One record of cnl_merge_tiles_f32's `views` table (32 bytes)."""
    _fields_ = [("frame_w", c_int32), ("frame_h", c_int32), ("x0", c_int32), ("y0", c_int32), ("pad_left", c_int32), ("pad_top", c_int32),
                ("sx", c_float), ("sy", c_float)]


class FlipMap(Structure):
    """cnl_flip_map: one head map of cnl_flip_merge_f32 (128 bytes): the two halves of the doubled batch and the destination, each a
    pointer with the element strides of the logical axes (n, c, y, x)."""
    _fields_ = [("a", c_void_p), ("a_sn", c_int64), ("a_sc", c_int64), ("a_sh", c_int64), ("a_sw", c_int64),
                ("b", c_void_p), ("b_sn", c_int64), ("b_sc", c_int64), ("b_sh", c_int64), ("b_sw", c_int64),
                ("dst", c_void_p), ("d_sn", c_int64), ("d_sc", c_int64), ("d_sh", c_int64), ("d_sw", c_int64),
                ("C", c_int32), ("swap_lr", c_int32)]


class MotTables(Structure):
    """cnl_mot_tables: the pooled input of one tracking evaluation — device pointers, then sizes; every member is 8 bytes."""
    POINTERS = ("gt_boxes", "pr_boxes", "gt_ids", "pr_ids", "gt_off", "pr_off", "sim_off", "frm_seq", "seq_frm", "seq_gid", "seq_tid", "seq_pair",
                "seq_idm", "gt_count", "pr_count")
    SCALARS = ("F", "S", "n_gt", "n_pr", "sim_total", "pair_total", "sum_g", "sum_t", "id_total", "max_gids", "max_gt_frame", "max_pr_frame",
               "max_frame_pairs")
    _fields_ = [(n, c_void_p) for n in POINTERS] + [(n, c_int64) for n in SCALARS]


class TrackGate(Structure):
    """cnl_track_gate: the gate operands of cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32 (40 bytes); null members: that gate is off."""
    _fields_ = [("trk_label", c_void_p), ("kx", c_void_p), ("kP", c_void_p), ("motion_gate", c_double), ("motion_weight", c_double)]


class TrackRows(Structure):
    """cnl_track_rows: the per-row state arrays of the device life cycle (56 bytes), all device memory."""
    _fields_ = [(n, c_void_p) for n in ("track_id", "state", "birth_age", "inactive_age", "label", "box", "trk_off")]


class TrackLifecycle(Structure):
    """cnl_track_lifecycle: the operands of cnl_track_lifecycle_i32 / cnl_track_lifecycle_emit_f64 (320 bytes)."""
    _fields_ = [("old_rows", TrackRows), ("new_rows", TrackRows), ("record", c_void_p), ("record_stride", ctypes.c_int64)] + \
               [(n, c_void_p) for n in ("live", "slot_of", "det_label", "det_box", "next_track_id", "status", "src_trk", "src_det", "flags", "keep_emb",
                                        "trk_eligible", "kalman_box", "out_box", "out_track_id", "out_label", "out_count", "workspace")] + \
               [("workspace_bytes", ctypes.c_int64)] + \
               [(n, c_int32) for n in ("S", "S_live", "k", "max_tracks", "label_kind", "low_record", "min_birth_age", "max_inactive_age", "step",
                                       "out_box_f64", "reset_stream", "reserved")]


class MotionFrame(Structure):
    """cnl_motion_frame: one frame record of cnl_camera_motion_u8 (40 bytes)."""
    _fields_ = [("src", c_void_p), ("cur", c_void_p), ("prev", c_void_p), ("h", c_int32), ("w", c_int32), ("row_stride", c_int32), ("reserved", c_int32)]


class CameraMotion(Structure):
    """cnl_camera_motion: the operands and the rule of one cnl_camera_motion_u8 call (112 bytes)."""
    _fields_ = [(n, c_void_p) for n in ("frames", "boxes", "count", "shift", "used", "vectors", "sad", "status")] + \
               [(n, c_int32) for n in ("L", "k", "step", "downscale", "gy", "gx", "block", "radius", "min_texture", "max_sad", "min_blocks", "reserved")]


class TrackZones(Structure):
    """cnl_track_zones: the operands and the rule of one cnl_track_zones_f64 call (168 bytes)."""
    _fields_ = [(n, c_void_p) for n in ("boxes", "track_ids", "labels", "count", "live", "geometry", "state", "status", "inside", "dwell", "occupancy",
                                        "zone_counts", "line_counts", "events", "event_count")] + \
               [(n, c_int32) for n in ("S", "L", "M", "max_tracks", "Z", "Ln", "max_events", "max_absent", "anchor", "boxes_f64", "bank", "step")]


class LossParams(Structure):
    """cnl_loss_params: the rule of one cnl_detection_loss_f64 call (72 bytes; cnl_sizeof_params(4))."""
    _fields_ = [("stride", c_double), ("target_param", c_double), ("hm_alpha", c_double), ("hm_beta", c_double),
                ("heatmap_weight", c_double), ("box_weight", c_double), ("box_multiplier", c_float), ("target_method", c_int32),
                ("heatmap_loss", c_int32), ("box_loss", c_int32), ("box_log", c_int32), ("reserved", c_int32)]


class ReidLossParams(Structure):
    """cnl_reid_loss_params: the rule of one cnl_reid_loss_f64 / cnl_reid_loss_grad_f32 call (48 bytes; cnl_sizeof_params(5))."""
    _fields_ = [("stride", c_double), ("bn_eps", c_double), ("momentum", c_double), ("ignore_index", c_int64), ("center", c_int32),
                ("padded_rows", c_int32), ("training", c_int32), ("reserved", c_int32)]


class AugmentPlacement(Structure):
    """cnl_augment_placement: one placement of an augmentation plan (96 bytes): a window of a source frame, where it goes in the canvas,
    whether it is mirrored, and its Q12 colour matrix."""
    _fields_ = [("frame", c_int32), ("x0", c_int32), ("y0", c_int32), ("w", c_int32), ("h", c_int32), ("dx0", c_int32), ("dy0", c_int32),
                ("dw", c_int32), ("dh", c_int32), ("flip", c_int32), ("colour", c_int32 * 12), ("reserved", c_int32 * 2)]


class WarpPlacement(Structure):
    """cnl_warp_placement: one placement of an affine augmentation plan (192 bytes): the clip window in a source frame, where it goes in the
    canvas, its Q12 colour matrix, the Q20 inverse map (canvas pixel -> source pixel index) and the float64 forward map."""
    _fields_ = [("frame", c_int32), ("x0", c_int32), ("y0", c_int32), ("w", c_int32), ("h", c_int32), ("dx0", c_int32), ("dy0", c_int32),
                ("dw", c_int32), ("dh", c_int32), ("reserved0", c_int32), ("colour", c_int32 * 12), ("inv", c_int64 * 6), ("fwd", c_double * 6),
                ("reserved", c_int32 * 2)]


class PixelOp(Structure):
    """cnl_pixel_op: the operation of one canvas of a pixel-level augmentation plan (400 bytes): its code, its parameter and the taps
    (dx, dy, w) of a filter."""
    _fields_ = [("op", c_int32), ("param", c_int32), ("n_taps", c_int32), ("reserved", c_int32), ("taps", (c_int32 * 3) * 32)]


assert ctypes.sizeof(LetterboxFrame) == 40 and ctypes.sizeof(AugmentPlacement) == 96 and ctypes.sizeof(WarpPlacement) == 192
assert ctypes.sizeof(PixelOp) == 400
assert ctypes.sizeof(MotionFrame) == 40 and ctypes.sizeof(CameraMotion) == 112
assert ctypes.sizeof(TrackZones) == 168

_REID_COMMON = [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, POINTER(ReidLossParams)]

_SIGNATURES = {
    "cnl_version": (ctypes.c_int, []),
    "cnl_sizeof_params": (c_size_t, [ctypes.c_int32]),
    "cnl_absmax_stride": (ctypes.c_int, []),
    "cnl_last_error": (c_size_t, [c_char_p, c_size_t]),
    "cnl_conv2d_nhwc_f32": (ctypes.c_int, [POINTER(ConvParams), c_void_p]),
    "cnl_fused_out_pack_weights_f32": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int32, ctypes.c_int32, c_void_p]),
    "cnl_fused_out_reduce_f32": (ctypes.c_int, [c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, c_void_p, c_void_p, ctypes.c_int32, ctypes.c_uint32, c_void_p]),
    "cnl_pointwise_nhwc_f32": (ctypes.c_int, [POINTER(ConvParams), c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "cnl_conv2d_out_hw": (ctypes.c_int, [POINTER(ConvParams), POINTER(c_int32), POINTER(c_int32)]),
    "cnl_conv3x3_winograd_f32": (ctypes.c_int, [POINTER(ConvParams), c_void_p]),
    "cnl_conv3x3_winograd_kernel": (ctypes.c_int, [POINTER(ConvParams)]),
    "cnl_winograd_up_weight_floats": (c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "cnl_winograd_transform_weights_up_f32": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int32, ctypes.c_int32, c_void_p]),
    "cnl_conv3x3_winograd_variant": (ctypes.c_int, [POINTER(ConvParams)]),
    "cnl_conv2d_kernel": (ctypes.c_int, [POINTER(ConvParams)]),
    "cnl_up2_weight_floats": (c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "cnl_up2_pack_weights_f32": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int32, ctypes.c_int32, c_void_p]),
    "cnl_conv3x3_up2_nhwc_f32": (ctypes.c_int, [POINTER(ConvParams), c_void_p]),
    "cnl_conv3x3_up2_kernel": (ctypes.c_int, [POINTER(ConvParams)]),
    "cnl_absmax_per_image_f32": (ctypes.c_int, [c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_void_p, c_void_p]),
    "cnl_winograd_weight_floats": (c_size_t, [c_int32, c_int32]),
    "cnl_winograd_transform_weights_f32": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "cnl_deconv2x_nhwc_f32": (ctypes.c_int, [POINTER(DeconvParams), c_void_p]),
    "cnl_deconv_phase_geometry": (ctypes.c_int, [c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]),
    "cnl_deconv_weight_floats": (c_size_t, [c_int32, c_int32, c_int32]),
    "cnl_conv2d_splitk_scratch_bytes": (c_size_t, [POINTER(ConvParams)]),
    "cnl_fuse_sum_nhwc_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_int32, c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_int32, c_void_p]),
    "cnl_upsample2x_nhwc_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                               c_int32, c_int32, c_void_p]),
    "cnl_depthwise3x3_nhwc_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                 c_int32, c_uint32, c_void_p]),
    "cnl_deform_sample_nhwc_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                  c_int32, c_int32, c_void_p]),
    "cnl_normalize_u8_nhwc_f32": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_float), POINTER(c_float), c_void_p]),
    "cnl_resize_bilinear_u8": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_letterbox_bilinear_u8": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_uint32, c_void_p]),
    "cnl_letterbox_yuv420_u8": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), c_uint32, c_void_p]),
    "cnl_unletterbox_boxes_f32": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_crop_boxes_u8": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), c_float,
                                         c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint32, c_void_p]),
    "cnl_draw_boxes_u8": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                         c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "cnl_flip_merge_f32": (ctypes.c_int, [POINTER(FlipMap), c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_mirror_append_u8": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_merge_tiles_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_merge_tiles_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                           c_float, c_float, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    "cnl_merge_soft_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_merge_soft_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                          c_float, c_int32, c_float, c_float, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_size_t, c_void_p]),
    "cnl_coco_match_f64": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cnl_coco_accumulate_f64": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "cnl_mot_similarity_f64": (ctypes.c_int, [POINTER(MotTables), c_void_p, c_void_p]),
    "cnl_mot_hota_workspace_bytes": (c_int64, [POINTER(MotTables)]),
    "cnl_mot_hota_f64": (ctypes.c_int, [POINTER(MotTables), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "cnl_mot_clear_workspace_bytes": (c_int64, [POINTER(MotTables)]),
    "cnl_mot_clear_f64": (ctypes.c_int, [POINTER(MotTables), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "cnl_mot_identity_workspace_bytes": (c_int64, [POINTER(MotTables)]),
    "cnl_mot_identity_f64": (ctypes.c_int, [POINTER(MotTables), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "cnl_detection_loss_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_detection_loss_f64": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                              c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, POINTER(LossParams),
                                              c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                              c_void_p]),
    "cnl_detection_loss_grad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_detection_loss_grad_f32": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                                   c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, POINTER(LossParams),
                                                   c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                                   c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cnl_reid_loss_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "cnl_reid_loss_f64": (ctypes.c_int, _REID_COMMON + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cnl_reid_loss_grad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "cnl_reid_loss_grad_f32": (ctypes.c_int, _REID_COMMON + [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                                              c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cnl_augment_u8": (ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_uint32, c_uint32,
                                      c_void_p]),
    "cnl_augment_boxes_f64": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_int32, c_double, c_double, c_void_p]),
    "cnl_augment_warp_u8": (ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_uint32, c_uint32,
                                           c_uint32, c_void_p]),
    "cnl_augment_warp_boxes_f64": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_double, c_double, c_void_p]),
    "cnl_augment_pixel_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "cnl_augment_pixel_u8": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_uint32, c_void_p, c_void_p, c_size_t,
                                            c_void_p]),
    "cnl_stem_conv7x7_u8": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, POINTER(c_float), POINTER(c_float), c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_stem_packed_weight_floats": (c_size_t, []),
    "cnl_stem_pack_weights_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    "cnl_stem_conv7x7_f32": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int32, c_int32, c_int32, c_uint32, c_void_p]),
    "cnl_stem_conv7x7_maxpool_f32": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int32, c_int32, c_int32, c_void_p]),
    "cnl_maxpool3x3s2_nhwc_f32": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_decode_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "cnl_decode_f32": (ctypes.c_int, [POINTER(DecodeParams), c_void_p]),
    "cnl_decode_forms": (ctypes.c_int, [POINTER(DecodeParams), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "cnl_gather_boxes_f32": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                            c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_void_p]),
    "cnl_gather_embeddings_f32": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                                 c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_pack_detections_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_unpack_detections_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_boxes_xyxy_to_xywh_f32": (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "cnl_track_costs_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_int32,
                                           c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cnl_track_costs_metric_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_int32,
                                                  c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cnl_track_apply_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_double,
                                           c_void_p, c_void_p, c_void_p]),
    "cnl_track_kalman_out_bytes": (ctypes.c_int64, [c_int32]),
    "cnl_track_kalman_f64": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    "cnl_conv_split_weight_floats": (ctypes.c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_conv_split_weights_f32": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_track_frame_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "cnl_track_frame_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p,
                                           c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_int64, c_void_p]),
    "cnl_lsap_batch_f64": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cnl_track_streams_workspace_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "cnl_track_streams_record_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "cnl_track_streams_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_float,
                                             c_double, c_float, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                             ctypes.c_int64, c_void_p, ctypes.c_int64, c_void_p]),
    "cnl_track_frame_low_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "cnl_track_frame_low_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p,
                                               c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_int64, c_void_p]),
    "cnl_track_streams_low_workspace_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "cnl_track_streams_low_record_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "cnl_track_streams_low_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_float,
                                                 c_double, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                                 c_int32, c_int32, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, c_void_p]),
    "cnl_track_apply_keep_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_double,
                                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "cnl_track_frame_gated_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p,
                                                 c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_int64, ctypes.POINTER(TrackGate), c_void_p]),
    "cnl_track_streams_gated_f32": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_float,
                                                   c_double, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                                   c_int32, c_int32, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, ctypes.POINTER(TrackGate),
                                                   c_void_p]),
    "cnl_track_lifecycle_workspace_bytes": (ctypes.c_int64, [c_int32, c_int32]),
    "cnl_track_lifecycle_i32": (ctypes.c_int, [ctypes.POINTER(TrackLifecycle), c_void_p]),
    "cnl_track_lifecycle_emit_f64": (ctypes.c_int, [ctypes.POINTER(TrackLifecycle), c_void_p]),
    "cnl_track_shift_f64": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_camera_motion_u8": (ctypes.c_int, [ctypes.POINTER(CameraMotion), c_int32, c_void_p]),
    "cnl_track_zones_state_bytes": (ctypes.c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_track_zones_f64": (ctypes.c_int, [ctypes.POINTER(TrackZones), c_void_p]),
    "cnl_relu_grad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_relu_grad_terms": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "cnl_relu_grad_f32": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                         c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cnl_conv_wgrad_slices": (c_int64, [c_int32] * 7),
    "cnl_conv_wgrad_workspace_bytes": (c_size_t, [c_int32] * 7),
    "cnl_conv_wgrad_terms": (c_int64, [c_int32] * 7),
    "cnl_conv_wgrad_nhwc_f32": (ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                               c_int32, c_void_p, c_size_t, c_void_p]),
    "cnl_conv1x1_dgrad_nhwc_f32": (ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "cnl_host_alloc": (ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(c_void_p)]),
    "cnl_host_free": (ctypes.c_int, [c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class HipLibraryError(RuntimeError):
    pass


def lib_path():
    return os.environ.get("CENTERNET_GFX950_LIB", _LIB_PATH)


def load():
    """Load (once) and return the ctypes handle.  Raises HipLibraryError when the .so is missing —
    build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C csrc`."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise HipLibraryError(f"{_LIB_NAME} not found at {path}; the HIP extension is required (no CPU fallback). "
                              "Build it with __graft_entry__.build().")
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise HipLibraryError(f"cannot load {path}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{path} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.cnl_version() != ABI_VERSION:
        raise HipLibraryError(f"{path} has ABI version {lib.cnl_version()}, this binding expects {ABI_VERSION}: rebuild it "
                              "(__graft_entry__.build())")
    for which, struct in ((0, ConvParams), (1, DecodeParams), (2, DeconvParams), (4, LossParams), (5, ReidLossParams)):       # the binding's struct layouts against the library's
        if lib.cnl_sizeof_params(which) != ctypes.sizeof(struct):
            raise HipLibraryError(f"{path}: sizeof({struct.__name__}) is {lib.cnl_sizeof_params(which)} in the library, {ctypes.sizeof(struct)} in this binding")
    _lib = lib
    return lib


def last_error():
    buf = ctypes.create_string_buffer(512)
    load().cnl_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc, what=""):
    """Map the C ABI's error convention onto Python exceptions (reference: bare asserts / exceptions)."""
    if rc == 0:
        return
    msg = f"{what}: {last_error()}" if what else last_error()
    if rc in (CNL_E_BAD_ARG, CNL_E_UNSUPPORTED):
        raise ValueError(msg)
    raise RuntimeError(msg)


def stream(device):
    """The hipStream_t argument of an entry point: the device's current torch stream."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def absmax_stride():
    """Floats between the per-image slots of an x_absmax / y_absmax array (one 128-byte line per image: include/centernet_gfx950.h)."""
    return load().cnl_absmax_stride()


def absmax_buffer(n, device="cuda"):
    """A zeroed per-image maxima array for n images (n * absmax_stride() floats)."""
    import torch
    return torch.zeros((n * absmax_stride(),), device=device, dtype=torch.float32)


def absmax_pack(values):
    """Per-image maxima (a tensor of n floats) -> the strided array the kernels read."""
    buf = absmax_buffer(values.numel(), values.device)
    buf[::absmax_stride()] = values.to(buf.dtype)
    return buf


def absmax_values(buf, n=None):
    """The n per-image values of a strided maxima array."""
    v = buf[::absmax_stride()]
    return v if n is None else v[:n]
