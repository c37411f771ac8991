"""Test-only yardstick for the YUV 4:2:0 entry (numpy, int32): the colour conversion rule of cnl_letterbox_yuv420_u8, restated on
its own, and the composed references — the existing numpy rules of tests/letterbox_ref.py and tests/tiled_ref.py applied to the
converted frame (resize and tiling are not restated here).

The rule is OpenCV's cvtColor(COLOR_YUV2RGB_NV12 / COLOR_YUV2RGB_I420) arithmetic restated from its published code ("parity unpinned",
as oracle/decode_ref.resize_bilinear_u8 states for cv2.resize: OpenCV is not a dependency of the tests): every pixel takes the chroma
sample of its 2 x 2 block (nearest), and in 32-bit integers with 20 fractional bits, >> an arithmetic shift:
    yy = max(0, Y - y_off) * CY
    R = sat8((yy + (1 << 19) + CVR * (V - 128)) >> 20)
    G = sat8((yy + (1 << 19) + CVG * (V - 128) + CUG * (U - 128)) >> 20)
    B = sat8((yy + (1 << 19) + CUB * (U - 128)) >> 20)
"""
import numpy as np

import letterbox_ref
import tiled_ref

# OpenCV's ITUR_BT_601_* constants: 1.164, 1.596, -0.813, -0.391, 2.018 times 2^20, truncated; y_off = 16
BT601_LIMITED = (16, 1220542, 1673527, -852492, -409993, 2116026)
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def coefficients(matrix="bt601", full_range=False):
    """(y_off, CY, CVR, CVG, CUG, CUB).  bt601 limited: OpenCV's constants; otherwise round(c * 2**20) of the standard matrix
    (Kg = 1 - Kr - Kb; chroma scaled by 255 / 224 and luma by 255 / 219 for limited range; CY = 1 << 20, y_off = 0 for full range)."""
    if matrix == "bt601" and not full_range:
        return BT601_LIMITED
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    s = 1.0 if full_range else 255.0 / 224.0
    c = (2 * (1 - kr) * s, -2 * (1 - kr) * kr / kg * s, -2 * (1 - kb) * kb / kg * s, 2 * (1 - kb) * s)
    return (0 if full_range else 16, (1 << 20) if full_range else round(255.0 / 219.0 * 2 ** 20)) + tuple(round(v * 2 ** 20) for v in c)


def yuv420_to_rgb(y, u, v, matrix="bt601", full_range=False):
    """y [h, w], u and v [h / 2, w / 2] uint8 -> [h, w, 3] RGB uint8."""
    y_off, cy, cvr, cvg, cug, cub = coefficients(matrix, full_range)
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and u.shape == v.shape == (h // 2, w // 2)
    Y = np.asarray(y, dtype=np.int32)
    U = np.repeat(np.repeat(np.asarray(u, dtype=np.int32), 2, axis=0), 2, axis=1) - 128       # nearest: the 2 x 2 block's sample
    V = np.repeat(np.repeat(np.asarray(v, dtype=np.int32), 2, axis=0), 2, axis=1) - 128
    yy = np.maximum(Y - y_off, 0) * np.int32(cy) + np.int32(1 << 19)
    rgb = np.stack([(yy + cvr * V) >> 20, (yy + cvg * V + cug * U) >> 20, (yy + cub * U) >> 20], axis=-1)
    assert rgb.dtype == np.int32
    return np.clip(rgb, 0, 255).astype(np.uint8)


def letterbox_yuv420_ref(planes, height, width, fill, matrix="bt601", full_range=False):
    """planes: list of (y, u, v) -> (canvas [N, height, width, 3], geometry list): letterbox_ref.expected_canvas of the converted frames."""
    return letterbox_ref.expected_canvas([yuv420_to_rgb(y, u, v, matrix, full_range) for (y, u, v) in planes], height, width, fill)


def tile_yuv420_ref(planes, tile_h, tile_w, overlap, full_frame, fill, matrix="bt601", full_range=False):
    """-> (views [V, tile_h, tile_w, 3], records, frame_first_view, views list): tiled_ref's views of the converted frames (crops for the
    tiles, letterbox_ref.expected_canvas for the full-frame view)."""
    rgb = [yuv420_to_rgb(y, u, v, matrix, full_range) for (y, u, v) in planes]
    rec, ffv, views = tiled_ref.view_records([f.shape[:2] for f in rgb], tile_h, tile_w, overlap, full_frame, letterbox_ref.geometry)
    out = np.empty((len(views), tile_h, tile_w, 3), dtype=np.uint8)
    for i, (n, y0, x0, th, tw) in enumerate(views):
        if full_frame and i == ffv[n + 1] - 1:
            out[i] = letterbox_ref.expected_canvas([rgb[n]], tile_h, tile_w, fill)[0][0]
        else:
            out[i] = tiled_ref.crop_view(rgb[n], y0, x0, th, tw, tile_h, tile_w, fill)
    return out, rec, ffv, views


def to_nv12(y, u, v):
    """(y, u, v) -> the single [h * 3 / 2, w] NV12 array (Y rows, then rows of interleaved U V)."""
    h, w = y.shape
    return np.concatenate([y, np.stack([u, v], axis=-1).reshape(h // 2, w)], axis=0)


def to_i420(y, u, v):
    """(y, u, v) -> the single [h * 3 / 2, w] I420 array (Y, then the U plane, then the V plane, as flat bytes)."""
    h, w = y.shape
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(h * 3 // 2, w)


def random_planes(rng, h, w):
    """Planes over the full 0..255 range (every saturation branch of the rule runs)."""
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))
