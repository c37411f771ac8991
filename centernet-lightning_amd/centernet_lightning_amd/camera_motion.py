"""Camera-motion estimation on the GPU: the global image translation between each stream's previous and current frame, the input of
`TrackerBank(lifecycle="device")`'s `camera_motion=` option (BoT-SORT's and StrongSORT's camera-motion compensation, translation only).

`CameraMotion.update` takes the frames `detect_frames` / `crop_detections` take (packed uint8 RGB / RGBA or NV12 / I420 surfaces, mixed sizes,
any pitch, read in place and read once) and makes one call of cnl_camera_motion_u8 (csrc/camera_motion.hip): coarse luma, block search,
aggregate — three launches, one pinned upload of the frame records, no synchronisation.  The object keeps each stream's previous coarse luma
plane on the device, double-buffered.  The rule is integer throughout: it is stated in include/centernet_gfx950.h and restated in numpy by
tests/camera_motion_ref.py.
"""
import ctypes

import numpy as np
import torch

from . import _frames, _gather, _lib

STATUS_NO_PREVIOUS, STATUS_FEW_BLOCKS, STATUS_TOO_SMALL = 1, 2, 4       # bits of out["status"]


def _int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name}={v!r}: expected an integer in {lo}..{hi}")
    return int(v)


class CameraMotion:
    """The estimator for `num_streams` video streams.

        cm = CameraMotion(num_streams=S)
        out = cm.update(frames)                     # one frame per stream
        scale = torch.tensor([1 / width, 1 / height], device=dev)      # step_batch's boxes are normalised: one torch multiply
        bank.step_batch(images, camera_motion=out["shift"] * scale)

    downscale d in {1, 2, 4, 8}: the coarse plane averages d x d lumas.  grid (gy, gx), each 1..16: the blocks; block B in {8, 16} and radius R
    in 1..8, in coarse pixels: a block is matched against every shift in [-R, R]^2, so shifts up to R * d frame pixels are found, in steps of
    d.  A block abstains when it is flat (sum |cur - mean| < min_texture * B * B), matches badly (best SAD > max_sad * B * B) or has its centre
    inside one of `boxes` (the foreground mask); with fewer than min_blocks votes the shift is 0.  The three rule values are defaults of a
    stated rule, not measurements."""

    def __init__(self, num_streams, downscale=4, grid=(8, 8), block=16, radius=8, min_texture=4, max_sad=24, min_blocks=4):
        self.num_streams = _int("num_streams", num_streams, 1, 65535)
        if isinstance(downscale, bool) or downscale not in (1, 2, 4, 8):
            raise ValueError(f"downscale={downscale!r}: expected 1, 2, 4 or 8")
        if isinstance(block, bool) or block not in (8, 16):
            raise ValueError(f"block={block!r}: expected 8 or 16")
        try:
            gy, gx = grid
        except (TypeError, ValueError):
            raise ValueError(f"grid={grid!r}: expected (rows, columns)") from None
        self.downscale, self.block = int(downscale), int(block)
        self.grid = (_int("grid rows", gy, 1, 16), _int("grid columns", gx, 1, 16))
        self.radius = _int("radius", radius, 1, 8)
        self.min_texture, self.max_sad = _int("min_texture", min_texture, 0, 255), _int("max_sad", max_sad, 0, 255)
        self.min_blocks = _int("min_blocks", min_blocks, 1, 256)
        self._stream = None             # the stream of the last update (a call under another stream finishes it first)
        self.reset()

    def reset(self, stream=None):
        """Forget the previous frame of every stream (None) or of one: its next frame reports shift 0 with status bit 0.  Host state only: the
        planes stay allocated."""
        S = self.num_streams
        if stream is None:
            self._size = [None] * S         # (h, w) of the frame whose coarse plane is current, None: no previous frame
            self._planes = [[None, None] for _ in range(S)]
            self._cur = [0] * S
            return
        self._size[self._check_streams([stream], 1)[0]] = None

    def _check_streams(self, streams, L):
        S = self.num_streams
        live = list(range(S)) if streams is None else [int(x) for x in streams]
        if not live or any(x < 0 or x >= S for x in live) or len(set(live)) != len(live):
            raise ValueError(f"streams={streams!r}: expected distinct stream indices in 0..{S - 1}, at least one")
        if len(live) != L:
            raise ValueError(f"{L} frames for {len(live)} participating streams: expected one frame per stream")
        return live

    def update(self, frames, streams=None, pixel_format="rgb", boxes=None, count=None):
        """frames[i] is the next frame of stream streams[i] (default: stream i) -> dict of device tensors, for L = len(frames):
        "shift" [L, 2] float32 (dx, dy) in the frame's own pixels: the content moved by it since the stream's previous frame; "used" [L] int32,
        the blocks that voted; "vectors" [L, gy * gx, 2] int16, per-block (sx, sy) in coarse pixels; "sad" [L, gy * gx] int32, the best SAD, -1
        for a block that abstained; "status" [L] int32: bit 0 no previous frame (the stream's first, or a frame of another size than the
        previous one), bit 1 fewer than min_blocks votes, bit 2 frame too small for the grid.
        boxes: float32 [L, k, 4] x1 y1 x2 y2 in frame pixels on the frames' device, gated by count (int32 [L]) as in crop_detections: a block
        whose centre lies inside a live, finite box does not vote."""
        what = "CameraMotion.update"
        src = _frames.open_frames(frames, pixel_format, what, copy=_frames.ROWS)
        L = len(src)
        live = self._check_streams(streams, L)
        dev = src.check_device()
        step = 1 if src.kind == _frames.YUV else src.C
        if step not in (1, 3, 4) or (src.kind == _frames.PACKED and step == 1):
            raise ValueError(f"{what}: packed frames need 3 (RGB) or 4 (RGBA) channels, got {src.C}")
        k = 0
        if boxes is not None:
            k = _frames.check_boxes(boxes, L, dev, what)
            if k < 1:
                raise ValueError(f"{what}: boxes {tuple(boxes.shape)}: expected k >= 1")
        if count is not None:
            if boxes is None:
                raise ValueError(f"{what}: count is given together with boxes")
            count = _frames.per_slot(count, "count", torch.int32, (L,), dev, what)
        d, (gy, gx) = self.downscale, self.grid
        nb = gy * gx
        plain, _ = src.records(src.whole())
        lib = _lib.load()
        with torch.cuda.device(dev):
            cur_stream = torch.cuda.current_stream(dev)
            if self._stream is not None and self._stream != cur_stream:
                self._stream.synchronize()          # the previous call wrote the planes this one reads
            rec = np.zeros((L, 5), np.int64)
            for i, (s, (h, w), (address, pitch)) in enumerate(zip(live, src.sizes, plain)):
                need = max((h // d) * (w // d), 1)
                pair, p = self._planes[s], self._cur[s]
                if pair[1 - p] is None or pair[1 - p].numel() < need or pair[1 - p].device != dev:
                    pair[1 - p] = torch.empty(need, device=dev, dtype=torch.uint8)
                prev = pair[p].data_ptr() if self._size[s] == (h, w) else 0
                rec[i, :3] = address, pair[1 - p].data_ptr(), prev
                rec[i, 3:].view(np.int32)[:3] = h, w, pitch
            table = _gather.upload(rec.reshape(-1), dev)
            out = {"shift": torch.empty((L, 2), device=dev, dtype=torch.float32), "used": torch.empty((L,), device=dev, dtype=torch.int32),
                   "vectors": torch.empty((L, nb, 2), device=dev, dtype=torch.int16), "sad": torch.empty((L, nb), device=dev, dtype=torch.int32),
                   "status": torch.empty((L,), device=dev, dtype=torch.int32)}
            args = _lib.CameraMotion(table.data_ptr(), boxes.data_ptr() if boxes is not None else None, count.data_ptr() if count is not None else None,
                                     out["shift"].data_ptr(), out["used"].data_ptr(), out["vectors"].data_ptr(), out["sad"].data_ptr(),
                                     out["status"].data_ptr(), L, k, step, d, gy, gx, self.block, self.radius, self.min_texture, self.max_sad,
                                     self.min_blocks, 0)
            _lib.check(lib.cnl_camera_motion_u8(ctypes.byref(args), 7, _lib.stream(dev)), "cnl_camera_motion_u8")
            self._stream = cur_stream
        for s, size in zip(live, src.sizes):
            self._size[s] = tuple(size)
            self._cur[s] = 1 - self._cur[s]
        return out
