"""`CenterNet` / `build_centernet()` — the drop-in boundary of the MI355X hot path.

Keeps the reference's Gen-A Python surface (README.md:29-37,94-101; docs/implementation.md:70-81;
tests/test_models.py:61-99; models/fairmot.py:138-151) with the Gen-B arithmetic that is actually in the
reference tree (models/meta.py:21-47, models/centernet.py:229-304):

    model = build_centernet("configs/base_resnet34_fpn.yaml").cuda().eval()
    heatmap, box_2d = model(images)                     # namedtuple; heatmap is post-sigmoid
    dets = model.gather_detection2d(heatmap, box_2d)    # {"bboxes","labels","scores"}

Everything between the input tensor and those outputs runs in libcenternet_gfx950.so (HIP, gfx950).
There is no CPU path: CPU tensors raise.  Training, datasets and evaluation stay with the reference.
"""
import ctypes
import math
from collections import OrderedDict, namedtuple
from typing import Any, Dict, Union

import torch
from torch import nn

from . import _lib
from . import coco_eval as _coco_eval
from . import conv_grad as _conv_grad
from . import crops as _crops
from . import decode as _decode
from . import flip as _flip
from . import letterbox as _letterbox
from . import loss as _loss
from . import overlay as _overlay
from . import tiles as _tiles
from .collate import collate_detections
from .config import model_section
from .engine import Engine
from .params import GenericHead, ResNetBackbone, build_neck

DetectionOutput = namedtuple("DetectionOutput", ["heatmap", "box_2d"])
TrackingOutput = namedtuple("TrackingOutput", ["heatmap", "box_2d", "reid"])

_HEAD_CHANNELS = {"box_2d": lambda cfg: 4}


def _as_output(out):
    """The engine's output dict -> the namedtuple forward() and forward_uint8() return."""
    if "reid" in out:
        return TrackingOutput(out["heatmap"], out["box_2d"], out["reid"])
    return DetectionOutput(out["heatmap"], out["box_2d"])


def _merged_result(merged, dets, first_view):
    """What detect_tiled and detect_multiscale return: the merge's dict without "source", and for tracking models the embeddings it picks."""
    result = {key: merged[key] for key in ("bboxes", "labels", "scores", "count")}
    if "embeddings" in dets:
        result["embeddings"] = _tiles.pick_embeddings(dets["embeddings"], merged["source"], first_view)
    return result


class _Head(GenericHead):
    """GenericHead parameters + the Gen-A per-head decode calls used by FairMOT.gather_tracking2d
    (models/fairmot.py:141-143)."""

    def __init__(self, name, in_channels, out_channels, model, **kw):
        super().__init__(in_channels, out_channels, **kw)
        self.head_name = name
        self._model_ref = [model]          # list: keep the parent out of the module tree

    # heads["heatmap"].gather_topk(heatmap, nms_kernel=3, num_detections=100) -> scores, indices, labels
    def gather_topk(self, heatmap, nms_kernel=3, num_detections=100):
        dummy_box = heatmap[:, :1].expand(-1, 4, -1, -1)          # strides only; the boxes are discarded
        out = _decode.decode(heatmap, dummy_box, None, num_detections, nms_kernel)
        return out["scores"], out["indices"], out["labels"]

    # heads["box_2d"].gather_at_indices(box_2d, indices, normalize_bbox=False, stride=4) / reid.gather_at_indices(reid, idx)
    def gather_at_indices(self, x, indices, normalize_bbox=False, stride=None):
        if self.head_name == "box_2d":
            m = self._model_ref[0]
            return _decode.gather_boxes(x, indices, normalize_bbox, m.box_log, m.box_multiplier,
                                        stride if stride is not None else m.output_stride)
        return _decode.gather_embeddings(x, indices)


class CenterNet(nn.Module):
    """CenterNet(backbone: dict, neck: dict, output_heads: dict, task: str, **ignored) — tests/test_models.py:62."""

    def __init__(self, backbone: Dict[str, Any], neck: Dict[str, Any], output_heads: Dict[str, Any], task: str = "detection",
                 num_detections: int = 100, nms_kernel: int = 3, box_log: bool = False, box_multiplier: float = 1.0,
                 **ignored):
        super().__init__()
        if task not in ("detection", "tracking"):
            raise ValueError(f"unknown task {task!r}")
        if "heatmap" not in output_heads:
            raise ValueError("output_heads must contain 'heatmap' (docs/implementation.md:60)")
        if "box_2d" not in output_heads:
            raise ValueError("output_heads must contain 'box_2d' for the detection/tracking decode")
        if task == "tracking" and "reid" not in output_heads:
            raise ValueError("task 'tracking' needs a 'reid' head (configs/base_tracking_resnet34_fpn.yaml:26-30)")
        self.task = task
        # the `model:` section this instance was built from (export.py rebuilds an identical model from it)
        self.config_section = {"backbone": dict(backbone), "neck": dict(neck), "output_heads": {k: dict(v or {}) for k, v in output_heads.items()},
                               "task": task, "num_detections": int(num_detections), "nms_kernel": int(nms_kernel), "box_log": bool(box_log),
                               "box_multiplier": float(box_multiplier)}
        self.backbone = ResNetBackbone(**backbone)
        self.neck = build_neck(neck, self.backbone.out_channels)
        self.output_stride = self.backbone.output_stride // self.neck.upsample_stride      # meta.py:96
        self.stride = self.output_stride
        self.num_classes = int(output_heads["heatmap"]["num_classes"])
        # Gen-B hyper-parameters of the decode (centernet.py:82-83,93-94)
        self.num_detections, self.nms_kernel = int(num_detections), int(nms_kernel)
        self.box_log, self.box_multiplier = bool(box_log), float(box_multiplier)
        # the validation loss's settings: Gen-A keys under output_heads.heatmap / .box_2d, Gen-B keys beside the decode's (loss.settings_from_config)
        self.loss_settings = _loss.settings_from_config(output_heads, **ignored)

        heads = OrderedDict()
        in_c = self.neck.out_channels
        for name, cfg in output_heads.items():
            cfg = dict(cfg or {})
            if name == "heatmap":
                out_c, d_width, d_depth = self.num_classes, 256, 3                       # meta.py:22
            elif name == "box_2d":
                out_c, d_width, d_depth = 4, 256, 3
            elif name == "reid":
                out_c, d_width, d_depth = int(cfg.get("emb_dim", 64)), 256, 1            # fairmot.py:20
            else:
                raise ValueError(f"output head '{name}' is outside the MI355X hot-path scope (heatmap, box_2d, reid)")
            heads[name] = _Head(name, in_c, out_c, self, width=int(cfg.get("width", d_width)),
                                depth=int(cfg.get("depth", d_depth)), init_bias=cfg.get("init_bias"))
        self.heads = nn.ModuleDict(heads)
        self._engine = Engine(self)
        self.eval()

    # ------------------------------------------------------------------ weights plumbing
    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._engine.invalidate()
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        if hasattr(self, "_engine"):
            self._engine.invalidate()
        return out

    def refresh_weights(self):
        """Force re-folding of BatchNorm and re-packing of the OHWI weights.  Not normally needed: the engine notices in-place
        writes to any parameter / buffer (version counters; e.g. model.backbone.load_state_dict(...)) before the next forward."""
        self._engine.invalidate()

    def set_kernel_options(self, **kw):
        """Kernel choice of the launch plan, explicit and per model (engine.KernelOptions): algo="auto" | "f2" | "f32", winograd,
        up2, absmax_handover, stem_fused_pool, reuse_buffers.  The HIP library reads no environment variables."""
        return self._engine.set_options(**kw)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("this CenterNet is the inference hot path only (eval-mode BatchNorm is folded into the HIP "
                               "kernels); training stays with the reference's Lightning module — except the heads over the frozen "
                               "trunk: head_trainer()")
        return super().train(False)

    # ------------------------------------------------------------------ fine-tuning the heads
    def neck_features(self, x: torch.Tensor) -> torch.Tensor:
        """The neck map the heads read, [N, C, H / stride, W / stride], as a fresh channels-last tensor: the plan run up to Plan.neck_out (where
        the plan folds a nearest-2x upsample into the first head blocks, the upsampled map).  No grad flows into it: the trunk is frozen."""
        return self._engine.neck_features(x)

    def head_trainer(self):
        """A conv_grad.HeadTrainer: an nn.Module whose parameters() are self.heads' own, and whose forward returns get_encoded_outputs' dict
        with a grad_fn (conv backward on the GPU, frozen BatchNorm statistics) — criterion()(trainer(x), targets)["total"].backward()."""
        return _conv_grad.HeadTrainer(self)

    # ------------------------------------------------------------------ forward
    def get_encoded_outputs(self, x: torch.Tensor, flip_test: bool = False) -> Dict[str, torch.Tensor]:
        """Forward pass returning a dict of logits (heatmap BEFORE sigmoid) — docs/implementation.md:77.
        flip_test: as in forward(); the heatmap LOGITS of the image and of its mirror are averaged."""
        if flip_test:
            return _flip.flip_merge(dict(self._engine.forward(_flip.mirror_append(x), sigmoid=False)), x.shape[0])
        return dict(self._engine.forward(x, sigmoid=False))

    get_output_dict = get_encoded_outputs          # alias used at utils/image_annotate.py:220, fairmot.py:88

    def forward(self, x: torch.Tensor, flip_test: bool = False):
        """namedtuple(heatmap after sigmoid, box_2d[, reid]) — docs/implementation.md:78; tests/test_models.py:88-99.
        flip_test: the flip test of the original CenterNet.  The network runs on 2N inputs, the images and their left-right mirrors
        (torch.cat((x, x.flip(-1))); the video path is forward_uint8), and every head map is the mean of the image's and the mirror's,
        mirrored back, before any decode (flip.flip_merge, one launch: the post-sigmoid heatmaps are averaged; box_2d swaps left and
        right and is averaged as the raw head output, which with box_log is a geometric mean of the sizes)."""
        if flip_test:
            return _flip.flip_merge(self.forward(_flip.mirror_append(x)), x.shape[0])
        return _as_output(self._engine.forward(x, sigmoid=True))

    # ------------------------------------------------------------------ step before the path
    IMAGENET_MEAN = (0.485, 0.456, 0.406)      # datasets/utils.py:9-10 of the reference
    IMAGENET_STD = (0.229, 0.224, 0.225)

    def preprocess_uint8(self, images: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
        """uint8 RGB frames [N,H,W,3] on the GPU -> normalised fp32 batch, logical [N,3,H,W] (channels_last storage, read
        zero-copy by forward()).  Same arithmetic as albumentations A.Normalize + ToTensorV2 (README.md:79-87)."""
        if not (isinstance(images, torch.Tensor) and images.is_cuda):
            raise RuntimeError("preprocess_uint8 runs on HIP devices only (no CPU fallback)")
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"expected uint8 [N,H,W,3], got {images.dtype} {tuple(images.shape)}")
        images = images.contiguous()
        N, H, W, _ = images.shape
        m, r = self._norm_constants(mean, std)
        with torch.cuda.device(images.device):
            out = torch.empty((N, H, W, 3), device=images.device, dtype=torch.float32)
            _lib.check(_lib.load().cnl_normalize_u8_nhwc_f32(images.data_ptr(), out.data_ptr(), N, H, W, m, r, _lib.stream(images.device)),
                       "cnl_normalize_u8_nhwc_f32")
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def _norm_constants(mean, std):
        import numpy as np
        m = np.array(mean, dtype=np.float32) * np.float32(255.0)
        r = np.reciprocal(np.array(std, dtype=np.float32) * np.float32(255.0), dtype=np.float32)
        return (ctypes.c_float * 3)(*m.tolist()), (ctypes.c_float * 3)(*r.tolist())

    def resize_uint8(self, images: torch.Tensor, height: int, width: int) -> torch.Tensor:
        """albumentations A.Resize(height, width) (README.md:84) = cv2.resize(..., INTER_LINEAR) on uint8 frames [N,H,W,C] -> [N,height,width,C]
        (cnl_resize_bilinear_u8: OpenCV's 8-bit fixed-point rule, bit-exact against oracle/decode_ref.resize_bilinear_u8)."""
        if not (isinstance(images, torch.Tensor) and images.is_cuda):
            raise RuntimeError("resize_uint8 runs on HIP devices only (no CPU fallback)")
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] > 4:
            raise ValueError(f"expected uint8 [N,H,W,C<=4], got {images.dtype} {tuple(images.shape)}")
        images = images.contiguous()
        N, H, W, C = images.shape
        lib = _lib.load()
        with torch.cuda.device(images.device):
            out = torch.empty((N, int(height), int(width), C), device=images.device, dtype=torch.uint8)
            _lib.check(lib.cnl_resize_bilinear_u8(images.data_ptr(), out.data_ptr(), N, H, W, int(height), int(width), C,
                                                  _lib.stream(images.device)), "cnl_resize_bilinear_u8")
        return out

    def forward_uint8(self, images: torch.Tensor, resize=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, flip_test: bool = False):
        """The reference's inference pre-processing fused into the path (README.md:79-101): uint8 HWC frames [N,H,W,3] ->
        [A.Resize(*resize) ->] A.Normalize -> forward().  The normalisation happens on the stem kernel's staged patch
        (cnl_stem_conv7x7_u8), so no fp32 image tensor is ever written: bit-identical to forward(preprocess_uint8(images)).
        flip_test: as in forward(); the (resized) frames are doubled by flip.mirror_append_uint8 (one launch) and the 2N outputs merged
        by flip.flip_merge (one launch)."""
        if resize is not None:
            images = self.resize_uint8(images, int(resize[0]), int(resize[1]))
        if flip_test:
            return _flip.flip_merge(self.forward_uint8(_flip.mirror_append_uint8(images), mean=mean, std=std), images.shape[0])
        m, r = self._norm_constants(mean, std)
        return _as_output(self._engine.forward_u8(images.contiguous(), m, r, sigmoid=True))

    # ------------------------------------------------------------------ frames of different sizes
    def letterbox_uint8(self, frames, height: int, width: int, fill=(0, 0, 0)):
        """uint8 frames of DIFFERENT sizes (a sequence of [h_i, w_i, 3] tensors on the GPU, or one [N,h,w,3] tensor) -> (canvas
        [N,height,width,3] uint8, geom): keep-aspect cv2 INTER_LINEAR resize (albumentations LongestMaxSize) centred on a constant `fill`
        border (PadIfNeeded(position="center")), one launch of cnl_letterbox_bilinear_u8 for the whole batch.  `geom` holds the device
        table and the host-side list of (h, w, new_h, new_w, pad_top, pad_left); see letterbox_geometry for the rule."""
        return _letterbox.letterbox_uint8(frames, height, width, fill)

    def unletterbox(self, bboxes: torch.Tensor, geom, clip: bool = True) -> torch.Tensor:
        """Boxes [N,k,4] in canvas pixels (gather_* with normalize_bbox=False) -> each frame's own pixels (cnl_unletterbox_boxes_f32)."""
        return _letterbox.unletterbox(bboxes, geom, clip)

    def letterbox_yuv420(self, frames, height: int, width: int, layout: str = "nv12", matrix: str = "bt601", full_range: bool = False,
                         fill=(0, 0, 0)):
        """letterbox_uint8 for YUV 4:2:0 video surfaces (NV12 / I420 planes of any pitch): the colour conversion happens inside the one
        launch (cnl_letterbox_yuv420_u8), no RGB frame is written; see letterbox.letterbox_yuv420."""
        return _letterbox.letterbox_yuv420(frames, height, width, layout, matrix, full_range, fill)

    def detect_frames(self, frames, height: int = 512, width: int = 512, fill=(0, 0, 0), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                      num_detections: int = 100, nms_kernel: int = 3, pixel_format: str = "rgb", matrix: str = "bt601",
                      full_range: bool = False, flip_test: bool = False):
        """Frames of different sizes -> {"bboxes" (each frame's own pixels, clipped to it), "labels", "scores"[, "embeddings"]}:
        letterbox_uint8 -> forward_uint8 on the canvas (the stem normalises: still no fp32 image in memory) -> the decode ->
        unletterbox.  Nothing between the frames and the result touches the host except the table upload.
        pixel_format "nv12" / "i420": the frames are YUV 4:2:0 surfaces (letterbox_yuv420 in place of letterbox_uint8; `matrix` and
        `full_range` choose the conversion); "rgb" ignores both.
        flip_test: forward_uint8's; the CANVAS is mirrored, after the letterbox, so the geometry table and unletterbox are untouched."""
        canvas, geom = _letterbox.letterbox_frames(frames, height, width, fill, pixel_format, matrix, full_range)
        dets = self._detect_views(canvas, "detect_frames", mean, std, flip_test, num_detections, nms_kernel)
        _letterbox.unletterbox_(dets["bboxes"], geom, True)
        return dets

    def _detect_views(self, views_u8, who, mean, std, flip_test, num_detections, nms_kernel):
        """The step detect_frames, detect_tiled (per chunk) and detect_multiscale (per scale) share: uint8 views [V, h, w, 3] -> forward_uint8
        -> the decode of the model's kind, boxes in view pixels."""
        if views_u8.shape[-1] != 3:
            raise ValueError(f"{who} expects 3-channel frames, got {views_u8.shape[-1]} channels")
        out = self.forward_uint8(views_u8, mean=mean, std=std, flip_test=flip_test)
        gather = self.gather_tracking2d if len(out) == 3 else self.gather_detection2d
        return gather(out, num_detections=num_detections, nms_kernel=nms_kernel, normalize_bbox=False)

    def crop_detections(self, frames, bboxes, size=(128, 64), scores=None, score_threshold=None, count=None, pad: float = 0.0,
                        keep_aspect: bool = False, fill=(0, 0, 0), pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False):
        """The boxes detect_frames / detect_tiled returned, cut out of the same frames at one size for a second-stage network ->
        (crops [N,k,size[0],size[1],C] uint8, windows [N,k,4] int32 x0 y0 w h), on the GPU (cnl_crop_boxes_u8); see crops.crop_detections."""
        return _crops.crop_detections(frames, bboxes, size, scores, score_threshold, count, pad, keep_aspect, fill, pixel_format, matrix,
                                      full_range)

    def draw_detections(self, frames, bboxes, labels=None, scores=None, score_threshold=None, count=None, numbers=None,
                        palette=_overlay.DEFAULT_PALETTE, text_color=(255, 255, 255), thickness: int = 2, fill_alpha: int = 0,
                        tag_scale: int = 2, pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False, inplace: bool = False):
        """The boxes detect_frames / detect_tiled returned, drawn onto the same frames (outlines, optional fills and number tags) on
        the GPU (cnl_draw_boxes_u8) -> the painted frames, in the form they were given; see overlay.draw_detections."""
        return _overlay.draw_detections(frames, bboxes, labels, scores, score_threshold, count, numbers, palette, text_color, thickness,
                                        fill_alpha, tag_scale, pixel_format, matrix, full_range, inplace)

    # ------------------------------------------------------------------ frames larger than the network input
    def tile_uint8(self, frames, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2, full_frame: bool = True, fill=(0, 0, 0)):
        """uint8 frames -> (views [V,tile_h,tile_w,C] uint8, geom): each frame's overlapping tiles (tile_grid) and, with full_frame, the
        whole frame letterboxed, gathered by one launch of cnl_letterbox_bilinear_u8; see tiles.tile_uint8."""
        return _tiles.tile_uint8(frames, tile_h, tile_w, overlap, full_frame, fill)

    def tile_yuv420(self, frames, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2, full_frame: bool = True, fill=(0, 0, 0),
                    layout: str = "nv12", matrix: str = "bt601", full_range: bool = False):
        """tile_uint8 for YUV 4:2:0 video surfaces, converted inside the one launch; see tiles.tile_yuv420."""
        return _tiles.tile_yuv420(frames, tile_h, tile_w, overlap, full_frame, fill, layout, matrix, full_range)

    def merge_tiles(self, bboxes, scores, labels, geom, **kwargs):
        """The detections of all views -> per frame, in its own pixels, duplicates removed (cnl_merge_tiles_f32); see tiles.merge_tiles."""
        return _tiles.merge_tiles(bboxes, scores, labels, geom, **kwargs)

    def detect_tiled(self, frames, tile=(512, 512), overlap: float = 0.2, full_frame: bool = True, batch: int = 32, fill=(0, 0, 0),
                     mean=IMAGENET_MEAN, std=IMAGENET_STD, num_detections: int = 100, nms_kernel: int = 3, max_detections: int = 300,
                     score_threshold: float = 0.1, match_threshold: float = 0.5, match_metric: str = "iou", class_aware: bool = True,
                     max_candidates: int = 4096, pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False,
                     flip_test: bool = False):
        """Sliced inference for frames larger than the network input -> {"bboxes" [N,max_detections,4] (each frame's own pixels),
        "labels", "scores", "count" [N] int32[, "embeddings"]}; rows past a frame's count are zero.
        tile_uint8 (one launch) -> forward_uint8 + the decode on chunks of at most `batch` views -> one merge over all frames
        (class-aware greedy NMS, IoU or intersection-over-smaller) -> for tracking models the embeddings of the survivors.
        Nothing between the frames and the result touches the host except the table upload.
        pixel_format "nv12" / "i420": the frames are YUV 4:2:0 surfaces (tile_yuv420 in place of tile_uint8), as in detect_frames.
        flip_test: forward_uint8's, on the gathered VIEWS (the tile table and merge_tiles are untouched): a chunk is still at most
        `batch` views, and its forward sees twice that many inputs."""
        _tiles.positive_int("detect_tiled", "batch", batch)
        views, geom = _tiles.tile_frames(frames, int(tile[0]), int(tile[1]), overlap, full_frame, fill, pixel_format, matrix, full_range)
        parts = [self._detect_views(views[i:i + batch], "detect_tiled", mean, std, flip_test, num_detections, nms_kernel)
                 for i in range(0, views.shape[0], batch)]
        dets = {key: (torch.cat([p[key] for p in parts]) if len(parts) > 1 else parts[0][key]) for key in parts[0]}
        m = _tiles.merge_tiles(dets["bboxes"], dets["scores"], dets["labels"], geom, max_detections=max_detections,
                               score_threshold=score_threshold, match_threshold=match_threshold, match_metric=match_metric,
                               class_aware=class_aware, max_candidates=max_candidates)
        return _merged_result(m, dets, geom.first_view)

    # ------------------------------------------------------------------ multi-scale test-time augmentation
    def merge_soft(self, bboxes, scores, labels, geom, **kwargs):
        """The detections of all views -> per frame, in its own pixels, merged by soft-NMS (cnl_merge_soft_f32); see tiles.merge_soft."""
        return _tiles.merge_soft(bboxes, scores, labels, geom, **kwargs)

    def detect_multiscale(self, frames, scales=(0.5, 0.75, 1.0, 1.25, 1.5), height: int = 512, width: int = 512, flip_test: bool = False,
                          method: str = "gaussian", sigma: float = 0.5, iou_threshold: float = 0.5, score_threshold: float = 0.001,
                          num_detections: int = 100, max_detections: int = 100, class_aware: bool = True, max_candidates: int = 4096,
                          nms_kernel: int = 3, fill=(0, 0, 0), mean=IMAGENET_MEAN, std=IMAGENET_STD, pixel_format: str = "rgb",
                          matrix: str = "bt601", full_range: bool = False):
        """The multi-scale test of the original CenterNet -> {"bboxes" [N,max_detections,4] (each frame's own pixels), "labels", "scores",
        "count" [N] int32[, "embeddings"]}; rows past a frame's count are zero.
        For every scale, in the order given: the frames letterboxed to that scale's canvas (letterbox.multiscale_sizes(height, width,
        scales): the canvas scaled and rounded to a multiple of 32) -> forward_uint8 -> the decode.  The S sets of detections are the S
        full-frame views of each frame: one soft-NMS merge over all frames puts them into the frame's pixels (tiles.merge_soft: method,
        sigma, iou_threshold, score_threshold, class_aware, max_candidates) -> for tracking models the embeddings of the picks.
        Nothing between the frames and the result touches the host except the table uploads (one per scale and one for the merge).
        Memory: each scale runs its own engine plan with its own arena; the default five scales take about 5.6 times the arena of scale
        1 (0.25 + 0.5625 + 1 + 1.5625 + 2.25), flip_test doubles that.  At most 8 scales (the engine keeps 8 plans).
        pixel_format, matrix, full_range, flip_test: as in detect_frames."""
        sizes = _letterbox.multiscale_sizes(height, width, scales)
        _tiles.check_soft_arguments("detect_multiscale", method, sigma, iou_threshold, score_threshold, max_detections, max_candidates)
        dets, views = self._detect_scales(frames, sizes, fill, mean, std, num_detections, nms_kernel, pixel_format, matrix, full_range, flip_test)
        m = _tiles.merge_soft(dets["bboxes"], dets["scores"], dets["labels"], views, method=method, sigma=sigma, iou_threshold=iou_threshold,
                              score_threshold=score_threshold, max_detections=max_detections, class_aware=class_aware,
                              max_candidates=max_candidates)
        return _merged_result(m, dets, views.first_view)

    def _detect_scales(self, frames, sizes, fill=(0, 0, 0), mean=IMAGENET_MEAN, std=IMAGENET_STD, num_detections: int = 100, nms_kernel: int = 3,
                       pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False, flip_test: bool = False):
        """What detect_multiscale merges (tools/multiscale_bench.py times the merge on it): per canvas size the frames letterboxed and
        _detect_views -> (the detections [N * S, k, ...], the views of a frame being its scales in the order given; their scale_geometry)."""
        parts, per_scale = [], []
        for (h_s, w_s) in sizes:
            canvas, geom = _letterbox.letterbox_frames(frames, h_s, w_s, fill, pixel_format, matrix, full_range)
            parts.append(self._detect_views(canvas, "detect_multiscale", mean, std, flip_test, num_detections, nms_kernel))
            per_scale.append(geom.frames)
        dets = {key: torch.stack([p[key] for p in parts], dim=1).flatten(0, 1) for key in parts[0]}           # [S][N, k, ...] -> [N * S, k, ...]
        return dets, _tiles.scale_geometry(per_scale, dets["bboxes"].device)

    # ------------------------------------------------------------------ decode (Gen-A names)
    def gather_detection2d(self, heatmap, box_2d=None, num_detections=100, nms_kernel=3, normalize_bbox=False):
        """-> {"bboxes": [N,k,4] x1y1x2y2, "labels": [N,k] i64, "scores": [N,k]} (README.md:58-64,97-101).
        Accepts the forward() namedtuple as the single argument.  `heatmap` is the post-sigmoid heatmap."""
        if box_2d is None and isinstance(heatmap, (tuple, list)):
            heatmap, box_2d = heatmap[0], heatmap[1]
        out = _decode.decode(heatmap, box_2d, None, num_detections, nms_kernel, normalize_bbox, self.box_log,
                             self.box_multiplier, self.output_stride)
        return {"bboxes": out["boxes"], "labels": out["labels"], "scores": out["scores"]}

    def gather_tracking2d(self, heatmap, box_2d=None, reid=None, num_detections=100, nms_kernel=3, normalize_bbox=False):
        """FairMOT.gather_tracking2d (fairmot.py:138-151): adds "embeddings": [N,k,E]."""
        if box_2d is None and isinstance(heatmap, (tuple, list)):
            heatmap, box_2d, reid = heatmap[0], heatmap[1], heatmap[2]
        out = _decode.decode(heatmap, box_2d, reid, num_detections, nms_kernel, normalize_bbox, self.box_log,
                             self.box_multiplier, self.output_stride)
        return {"bboxes": out["boxes"], "labels": out["labels"], "scores": out["scores"], "embeddings": out["embeddings"]}

    # ------------------------------------------------------------------ decode (Gen-B names, centernet.py:229-304)
    def decode_detections(self, heatmap, box_offsets, normalize_boxes=False):
        out = _decode.decode(heatmap, box_offsets, None, self.num_detections, self.nms_kernel, normalize_boxes, self.box_log,
                             self.box_multiplier, self.stride)
        return {"boxes": out["boxes"], "scores": out["scores"], "labels": out["labels"]}

    def get_topk_from_heatmap(self, heatmap, pseudo_nms=True):
        return self.heads["heatmap"].gather_topk(heatmap, self.nms_kernel if pseudo_nms else 1, self.num_detections)

    @staticmethod
    def gather_and_decode_boxes(box_offsets, indices, normalize_boxes=False, box_log=False, box_multiplier=1.0, stride=4):
        return _decode.gather_boxes(box_offsets, indices, normalize_boxes, box_log, box_multiplier, stride)

    def evaluator(self, device=None):
        """A CocoEvaluator for this model's classes: feed it gather_detection2d's dict and the targets, batch by batch (coco_eval.py)."""
        return _coco_eval.CocoEvaluator(self.num_classes, device)

    def compute_loss(self, outputs: Dict[str, torch.Tensor], targets, stride=None):
        """The reference's compute_loss (models/centernet.py:123-175) as a validation VALUE: outputs is the dict of get_encoded_outputs (heatmap
        logits), targets the reference's list of per-image {"boxes" x y w h, "labels"} or padded device tensors -> {"heatmap", "box_2d", "total"}
        (0-dim float64 device tensors), "per_image", "skipped" (loss.detection_loss).  Target method, loss functions and weights come from the
        config, stride / box_log / box_multiplier from the model; the reid loss is left out, as the reference leaves it out at validation
        (tracking_criterion() is the training criterion with it)."""
        return _loss.detection_loss(outputs["heatmap"], outputs["box_2d"], targets, **self._loss_kwargs(stride))

    def loss_meter(self):
        """A LossMeter with this model's loss settings: update(outputs, targets) per batch, get_metrics() at the end of the epoch (loss.py)."""
        return _loss.LossMeter(**self._loss_kwargs(None))

    def criterion(self):
        """A DetectionLoss with this model's loss settings: criterion(outputs, targets)["total"].backward() for a training step (loss.py)."""
        return _loss.DetectionLoss(**self._loss_kwargs(None))

    def tracking_criterion(self, max_track_ids=None):
        """A TrackingLoss for a tracking model: DetectionLoss with this model's settings plus a ReIDLoss built from output_heads.reid.{emb_dim,
        max_track_ids, loss_weight} (max_track_ids: overrides the config's, e.g. the identity count of the training set).  The ReIDLoss owns the
        training-only classifier: give its parameters to the optimizer and move it to the device (criterion.to(device))."""
        if self.task != "tracking":
            raise ValueError("tracking_criterion() needs a tracking model (task 'tracking' with a 'reid' head); a detection model's criterion is criterion()")
        cfg = dict(self.config_section["output_heads"].get("reid") or {})
        ids = cfg.get("max_track_ids", 1000) if max_track_ids is None else max_track_ids
        reid = _loss.ReIDLoss(int(cfg.get("emb_dim", 64)), int(ids), float(cfg.get("loss_weight", 1.0)), stride=self.stride)
        return _loss.TrackingLoss(self._loss_kwargs(None), reid)

    def _loss_kwargs(self, stride):
        return dict(self.loss_settings, stride=self.stride if stride is None else stride, box_log=self.box_log, box_multiplier=self.box_multiplier)

    # ------------------------------------------------------------------ multi-GPU
    def collate(self, detections: Dict[str, torch.Tensor], group=None):
        """All-gather this rank's detections over the process group (RCCL on HIP) — eval/coco.py:10-18 precedent."""
        return collate_detections(detections, group)


def build_centernet(config: Union[str, Dict[str, Any]]) -> CenterNet:
    """Build from a YAML path or a dict (README.md:31-37).  Reads the `model:` section only."""
    m = model_section(config)
    extra = {k: m[k] for k in ("num_detections", "nms_kernel", "box_log", "box_multiplier") + _loss.GEN_B_KEYS if k in m}
    return CenterNet(m["backbone"], m["neck"], m["output_heads"], m.get("task", "detection"), **extra)
