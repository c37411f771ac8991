"""No GPU: the letterbox geometry rule, the two new C-ABI entry points' declarations and argument checks, and the float64 helper the
GPU tests measure against (tests/letterbox_ref.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import letterbox_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnl_letterbox_bilinear_u8", "cnl_unletterbox_boxes_f32")
SIZES = [(1080, 1920), (720, 1280), (1920, 1080), (640, 640), (512, 512), (608, 1088), (7, 5), (1, 1), (16, 1200), (1200, 16), (333, 517),
         (1, 4000), (4000, 1), (5, 64), (7, 64), (511, 513), (97, 3), (2, 1)]
TARGETS = [(512, 512), (608, 1088), (32, 32), (96, 64)]


@pytest.mark.parametrize("height,width", TARGETS)
def test_geometry_fills_one_axis_stays_inside_and_centres(height, width):
    for h, w in SIZES:
        nh, nw, pt, pl = cl.letterbox_geometry(h, w, height, width)
        assert nh == height or nw == width, (h, w)
        assert 1 <= nh <= height and 1 <= nw <= width, (h, w)
        assert pt == (height - nh) // 2 and pl == (width - nw) // 2
        pb, pr = height - nh - pt, width - nw - pl
        assert pt + nh + pb == height and pl + nw + pr == width
        assert 0 <= pb - pt <= 1 and 0 <= pr - pl <= 1          # the odd pixel goes to the bottom / right
        assert (nh, nw, pt, pl) == letterbox_ref.geometry(h, w, height, width)
    assert cl.letterbox_geometry(height, width, height, width) == (height, width, 0, 0)


def test_geometry_rounds_half_to_even():
    # 5 x 64 -> 32 x 32: r = 0.5, h * r = 2.5 -> 2 (half-up would give 3); 7 x 64: 3.5 -> 4 under both rules
    assert cl.letterbox_geometry(5, 64, 32, 32) == (2, 32, 15, 0)
    assert cl.letterbox_geometry(7, 64, 32, 32) == (4, 32, 14, 0)
    assert cl.letterbox_geometry(64, 5, 32, 32) == (32, 2, 0, 15)


def test_geometry_extreme_frames():
    assert cl.letterbox_geometry(1, 1, 512, 512) == (512, 512, 0, 0)
    assert cl.letterbox_geometry(1, 4000, 512, 512) == (1, 512, 255, 0)          # round(0.128) = 0 -> at least one row
    assert cl.letterbox_geometry(4000, 1, 512, 512) == (512, 1, 0, 255)
    assert cl.letterbox_geometry(1, 4000, 608, 1088) == (1, 1088, 303, 0)


@pytest.mark.parametrize("args", [(0, 5, 512, 512), (5, 0, 512, 512), (-1, 5, 512, 512), (5, 5, 0, 512), (5, 5, 512, 500), (5, 5, 100, 512),
                                  (5, 5, -32, 32), (5.0, 5, 512, 512), (5, 5, 512.0, 512)])
def test_geometry_rejects_bad_arguments(args):
    with pytest.raises(ValueError):
        cl.letterbox_geometry(*args)


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/centernet_gfx950.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # entry points only: no ABI bump
    assert "cnl_letterbox_frame" in header and ctypes.sizeof(_lib.LetterboxFrame) == 40
    assert [(n, getattr(_lib.LetterboxFrame, n).offset) for n, _ in _lib.LetterboxFrame._fields_] == [
        ("src", 0), ("h", 8), ("w", 12), ("row_stride", 16), ("new_h", 20), ("new_w", 24), ("pad_top", 28), ("pad_left", 32), ("reserved", 36)]
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
        assert set(ENTRY_POINTS) <= defined


def test_entry_points_validate_arguments_without_a_device():
    lib = _lib.load()
    E = _lib.CNL_E_BAD_ARG
    fake = 0x10000          # never dereferenced: every call below fails validation first
    assert lib.cnl_letterbox_bilinear_u8(fake, fake, 1, 512, 512, 5, 0, None) == E and "C = 5" in _lib.last_error()
    assert lib.cnl_letterbox_bilinear_u8(fake, fake, 1, 512, 512, 0, 0, None) == E
    assert lib.cnl_letterbox_bilinear_u8(fake, fake, -1, 512, 512, 3, 0, None) == E and "N = -1" in _lib.last_error()
    assert lib.cnl_letterbox_bilinear_u8(None, fake, 1, 512, 512, 3, 0, None) == E and "null" in _lib.last_error()
    assert lib.cnl_letterbox_bilinear_u8(fake, None, 1, 512, 512, 3, 0, None) == E
    assert lib.cnl_letterbox_bilinear_u8(fake, fake, 1, 500, 512, 3, 0, None) == E and "multiple of 32" in _lib.last_error()
    assert lib.cnl_letterbox_bilinear_u8(fake, fake, 1, 512, 0, 3, 0, None) == E
    assert lib.cnl_letterbox_bilinear_u8(fake + 4, fake, 1, 512, 512, 3, 0, None) == E and "aligned" in _lib.last_error()
    assert lib.cnl_letterbox_bilinear_u8(None, None, 0, 512, 512, 3, 0, None) == 0           # an empty batch is a no-op
    assert lib.cnl_unletterbox_boxes_f32(fake, fake, -1, 10, 1, None) == E
    assert lib.cnl_unletterbox_boxes_f32(fake, fake, 1, -1, 1, None) == E
    assert lib.cnl_unletterbox_boxes_f32(None, fake, 1, 10, 1, None) == E and "null" in _lib.last_error()
    assert lib.cnl_unletterbox_boxes_f32(fake, None, 1, 10, 1, None) == E
    assert lib.cnl_unletterbox_boxes_f32(fake + 4, fake, 1, 10, 1, None) == E
    assert lib.cnl_unletterbox_boxes_f32(None, None, 0, 10, 1, None) == 0
    with pytest.raises(ValueError):
        _lib.check(E, "x")


def test_python_surface_rejects_cpu_and_malformed_frames():
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    for name in ("letterbox_uint8", "unletterbox", "detect_frames"):
        assert callable(getattr(model, name))
    with pytest.raises(RuntimeError):
        model.letterbox_uint8([torch.zeros((8, 8, 3), dtype=torch.uint8)], 32, 32)            # CPU frames: no fallback
    with pytest.raises(RuntimeError):
        model.detect_frames(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        model.unletterbox(torch.zeros((1, 4, 4)), None)
    with pytest.raises(ValueError):
        model.letterbox_uint8([], 32, 32)
    with pytest.raises(ValueError):
        model.letterbox_uint8(torch.zeros((8, 8, 3), dtype=torch.uint8), 32, 32)              # a tensor must be 4-D


def test_float64_unmap_inverts_the_forward_mapping():
    for (h, w) in SIZES:
        for (height, width) in TARGETS[:2]:
            g = (h, w) + letterbox_ref.geometry(h, w, height, width)
            xs, ys = np.meshgrid(np.linspace(0, w, 9), np.linspace(0, h, 7))
            pts = np.stack([xs.ravel(), ys.ravel()], axis=-1)
            a, b = letterbox_ref.letterbox_points(pts, g), letterbox_ref.letterbox_points(pts[::-1], g)
            boxes = np.concatenate([a, b], axis=-1)[None]                                     # [1, k, 4] in canvas pixels
            assert boxes[..., 0::2].min() >= g[5] - 1e-9 and boxes[..., 0::2].max() <= g[5] + g[3] + 1e-9      # inside the window
            assert boxes[..., 1::2].min() >= g[4] - 1e-9 and boxes[..., 1::2].max() <= g[4] + g[2] + 1e-9
            back = letterbox_ref.unletterbox_boxes(boxes, [g], clip=False)[0]
            np.testing.assert_allclose(back, np.concatenate([pts, pts[::-1]], axis=-1), rtol=0, atol=1e-9 * max(h, w))
            clipped = letterbox_ref.unletterbox_boxes(boxes + 1e4, [g], clip=True)[0]
            assert (clipped[:, 0::2] == w).all() and (clipped[:, 1::2] == h).all()
            assert (letterbox_ref.unletterbox_bound(boxes, [g]) >= 0).all()


def test_expected_canvas_helper_places_the_resized_frame_on_the_fill():
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (5, 64, 3), dtype=np.uint8), rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)]
    canvas, geo = letterbox_ref.expected_canvas(frames, 32, 32, (9, 8, 7))
    assert geo[0] == (5, 64, 2, 32, 15, 0) and geo[1] == (32, 32, 32, 32, 0, 0)
    assert (canvas[0, :15] == np.array([9, 8, 7], dtype=np.uint8)).all() and (canvas[0, 17:] == np.array([9, 8, 7], dtype=np.uint8)).all()
    assert np.array_equal(canvas[1], frames[1])                    # identity resize
