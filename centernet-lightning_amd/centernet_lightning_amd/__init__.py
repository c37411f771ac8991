"""centernet_lightning_amd — MI355X-native (gfx950) CenterNet inference hot path.

Drop-in for the detection hot path of gau-nernst/centernet-lightning: `build_centernet()`,
`CenterNet.forward()`, `gather_detection2d()` / `gather_tracking2d()`.  Python orchestrates; all compute
is in libcenternet_gfx950.so (hand-written HIP kernels, C ABI in include/centernet_gfx950.h).
"""
from .config import load_config
from .models import CenterNet, DetectionOutput, TrackingOutput, build_centernet
from .collate import (Collator, all_gather_records, collate_detections, pack_detections, shard_range, unpack_detections)
from .tracker import Tracker, TrackerBank, Track, TrackState, ResidentTrack, build_tracker, match_with_threshold
from . import decode, formats
from .letterbox import LetterboxGeometry, letterbox_geometry, letterbox_yuv420, multiscale_sizes
from .tiles import TileGeometry, merge_soft, merge_tiles, tile_grid, tile_uint8, tile_yuv420
from .yuv import rgb_to_yuv, split_planes, yuv_coefficients
from .crops import crop_detections
from .camera_motion import CameraMotion
from .zones import Line, Zone, ZoneCounter
from .overlay import DEFAULT_PALETTE, draw_detections
from .flip import flip_merge, mirror_append_uint8
from .coco_eval import CocoEvaluator
from .mot_eval import MotEvaluator, evaluate_mot_tracking_sequence
from .loss import (DetectionLoss, LossMeter, ReIDLoss, TrackingLoss, detection_loss, detection_loss_grad, reid_loss, reid_loss_grad, render_targets)
from .augment import AugmentPlan, TrainAugment, augment_batch, sample_augment
from .warp import TrainWarp, WarpPlan, affine_matrix, sample_warp, warp_batch, warp_inverse
from .pixel import PixelPlan, TrainTransform, motion_blur_taps, pixel_batch, sample_pixel, sharpen_taps
from .conv_grad import HeadTrainer, conv2d_nhwc
from .export import TraceableCenterNet, export_onnx, export_torchscript

__all__ = ["CenterNet", "build_centernet", "load_config", "DetectionOutput", "TrackingOutput", "decode",
           "collate_detections", "Collator", "all_gather_records", "pack_detections", "unpack_detections", "shard_range",
           "Tracker", "TrackerBank", "Track", "TrackState", "ResidentTrack", "build_tracker", "match_with_threshold", "formats", "TraceableCenterNet", "export_torchscript", "export_onnx",
           "letterbox_geometry", "LetterboxGeometry", "TileGeometry", "tile_grid", "tile_uint8", "merge_tiles",
           "letterbox_yuv420", "tile_yuv420", "yuv_coefficients", "split_planes", "crop_detections", "CameraMotion", "ZoneCounter", "Zone", "Line",
           "draw_detections", "DEFAULT_PALETTE", "rgb_to_yuv", "flip_merge", "mirror_append_uint8", "CocoEvaluator",
           "MotEvaluator", "evaluate_mot_tracking_sequence", "LossMeter", "detection_loss", "render_targets", "DetectionLoss",
           "detection_loss_grad", "reid_loss", "reid_loss_grad", "ReIDLoss", "TrackingLoss",
           "augment_batch", "sample_augment", "AugmentPlan", "TrainAugment",
           "warp_batch", "sample_warp", "WarpPlan", "TrainWarp", "affine_matrix", "warp_inverse",
           "pixel_batch", "sample_pixel", "PixelPlan", "TrainTransform", "motion_blur_taps", "sharpen_taps", "merge_soft", "multiscale_sizes",
           "HeadTrainer", "conv2d_nhwc"]
