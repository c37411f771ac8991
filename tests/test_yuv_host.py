"""No GPU: the YUV 4:2:0 conversion rule (tests/yuv_ref.py) and its integers, the three input forms, the refusals of the Python
surface, the geometry, and the new C-ABI entry point's declaration and argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import letterbox_ref
import tiled_ref
import yuv_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _gather, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cnl_letterbox_yuv420_u8"
COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


def one(Y, U, V, matrix="bt601", full_range=False):
    px = yuv_ref.yuv420_to_rgb(np.full((2, 2), Y, np.uint8), np.full((1, 1), U, np.uint8), np.full((1, 1), V, np.uint8), matrix, full_range)
    assert (px == px[0, 0]).all()
    return tuple(int(c) for c in px[0, 0])


# ----------------------------------------------------------------------------- the rule
def test_oracle_known_answers_bt601_limited():
    assert one(16, 128, 128) == (0, 0, 0)
    assert one(235, 128, 128) == (255, 255, 255)
    assert one(255, 128, 128) == (255, 255, 255)           # saturates
    for U, V in ((128, 128), (90, 240), (0, 255), (255, 0)):
        assert one(0, U, V) == one(16, U, V)               # below black is black
    assert one(81, 90, 240) == (254, 0, 0)                 # BT.601 red


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_oracle_is_monotone_in_y_at_fixed_chroma(matrix, full_range):
    ys = np.arange(256, dtype=np.uint8).reshape(2, 128)
    for U, V in ((128, 128), (0, 0), (255, 255), (0, 255), (255, 0), (90, 240), (37, 201)):
        rgb = yuv_ref.yuv420_to_rgb(ys, np.full((1, 64), U, np.uint8), np.full((1, 64), V, np.uint8), matrix, full_range).reshape(256, 3)
        assert (np.diff(rgb.astype(np.int32), axis=0) >= 0).all(), (matrix, full_range, U, V)
    grey = yuv_ref.yuv420_to_rgb(ys, np.full((1, 64), 128, np.uint8), np.full((1, 64), 128, np.uint8), matrix, full_range).reshape(256, 3)
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all()      # no chroma: grey
    if full_range:
        assert (grey[:, 0] == np.arange(256)).all()                                   # CY = 1: the identity


def test_bt601_limited_constants_are_opencvs():
    six = (16, 1220542, 1673527, -852492, -409993, 2116026)
    assert cl.yuv_coefficients() == six and cl.yuv_coefficients("bt601", False) == six
    assert yuv_ref.coefficients("bt601", False) == six
    for c, k in zip((1.164, 1.596, -0.813, -0.391, 2.018), six[1:]):                  # ... times 2^20, truncated
        assert k == int(c * 2 ** 20), (c, k)


@pytest.mark.parametrize("matrix,full_range", COMBOS[1:])
def test_other_matrices_are_the_rounded_standard_coefficients(matrix, full_range):
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    kg = 1.0 - kr - kb
    s = 1.0 if full_range else 255.0 / 224.0
    c = (2 * (1 - kr) * s, -2 * (1 - kr) * kr / kg * s, -2 * (1 - kb) * kb / kg * s, 2 * (1 - kb) * s)
    want = (0, 1 << 20) if full_range else (16, round(255.0 / 219.0 * 2 ** 20))
    want += tuple(round(v * 2 ** 20) for v in c)
    assert cl.yuv_coefficients(matrix, full_range) == want == yuv_ref.coefficients(matrix, full_range)
    # ... and those are the published decimals (full range: BT.601 1.402 / -0.714136 / -0.344136 / 1.772, BT.709 1.5748 / -0.4681 / -0.1873 / 1.8556)
    published = {"bt601": (1.402, -0.714136, -0.344136, 1.772), "bt709": (1.5748, -0.4681, -0.1873, 1.8556)}[matrix]
    for k, p in zip(want[2:], published):
        assert abs(k / 2 ** 20 - p * s) < 1e-4, (k, p)
    # 32-bit arithmetic cannot overflow (the C ABI's own condition)
    assert 255 * want[1] + (1 << 19) + 128 * max(abs(want[2]), abs(want[3]) + abs(want[4]), abs(want[5])) < 2 ** 31


# ----------------------------------------------------------------------------- input forms
def test_the_three_input_forms_parse_to_the_same_planes():
    rng = np.random.default_rng(0)
    for (h, w) in ((6, 8), (2, 2), (34, 20), (10, 6)):              # 10 x 6: the I420 chroma planes end in the middle of a row
        y, u, v = yuv_ref.random_planes(rng, h, w)
        ty, tu, tv = torch.from_numpy(y), torch.from_numpy(u), torch.from_numpy(v)
        uv = torch.stack([tu, tv], dim=-1)
        pitched_y = torch.zeros((h, w + 24), dtype=torch.uint8)
        pitched_y[:, :w] = ty
        pitched_uv = torch.zeros((h // 2, w // 2 + 5, 2), dtype=torch.uint8)
        pitched_uv[:, :w // 2] = uv
        surface = torch.zeros((h * 3 // 2, w + 32), dtype=torch.uint8)          # a decoder surface: pitch > width
        surface[:, :w] = torch.from_numpy(yuv_ref.to_nv12(y, u, v))
        forms = [(torch.from_numpy(yuv_ref.to_nv12(y, u, v)), "nv12"), (torch.from_numpy(yuv_ref.to_i420(y, u, v)), "i420"),
                 ((ty, uv), "nv12"), ((ty, tu, tv), "i420"), ((pitched_y[:, :w], pitched_uv[:, :w // 2]), "nv12"), (surface[:, :w], "nv12"),
                 ([ty, tu, tv], "nv12")]                                         # forms (b), (c) describe themselves: layout is for (a)
        for frame, layout in forms:
            py, pu, pv = cl.split_planes(frame, layout)
            assert torch.equal(py, ty) and torch.equal(pu, tu) and torch.equal(pv, tv), (h, w, layout)
        # views, not copies: the pitched planes are read in place
        py, pu, pv = cl.split_planes((pitched_y[:, :w], pitched_uv[:, :w // 2]), "nv12")
        assert py.data_ptr() == pitched_y.data_ptr() and pu.data_ptr() == pitched_uv.data_ptr() and pv.data_ptr() == pu.data_ptr() + 1
        py, pu, pv = cl.split_planes(surface[:, :w], "nv12")
        assert py.data_ptr() == surface.data_ptr() and pu.data_ptr() == surface.data_ptr() + h * (w + 32) and pv.data_ptr() == pu.data_ptr() + 1
        # the oracle's converted frame does not depend on the form either
        assert np.array_equal(yuv_ref.yuv420_to_rgb(py.numpy(), pu.numpy(), pv.numpy()), yuv_ref.yuv420_to_rgb(y, u, v))


def planes(h, w, dtype=torch.uint8, device="cpu"):
    return (torch.zeros((h, w), dtype=dtype, device=device), torch.zeros((h // 2, w // 2), dtype=dtype, device=device),
            torch.zeros((h // 2, w // 2), dtype=dtype, device=device))


BAD_FRAMES = {
    "odd height": (torch.zeros((5, 8), dtype=torch.uint8),) + planes(4, 8)[1:],
    "odd width": (torch.zeros((4, 7), dtype=torch.uint8), torch.zeros((2, 3), dtype=torch.uint8), torch.zeros((2, 3), dtype=torch.uint8)),
    "odd single": torch.zeros((9, 7), dtype=torch.uint8),                       # h = 6, w = 7
    "rows not 3/2": torch.zeros((10, 8), dtype=torch.uint8),
    "float": planes(4, 8, torch.float32),
    "float single": torch.zeros((6, 8), dtype=torch.float32),
    "u shape": (planes(4, 8)[0], torch.zeros((2, 3), dtype=torch.uint8), planes(4, 8)[2]),
    "v shape": (planes(4, 8)[0], planes(4, 8)[1], torch.zeros((1, 4), dtype=torch.uint8)),
    "uv shape": (planes(4, 8)[0], torch.zeros((2, 4, 3), dtype=torch.uint8)),
    "uv not interleaved": (planes(4, 8)[0], torch.zeros((2, 8), dtype=torch.uint8)),
    "y 3-d": (torch.zeros((4, 8, 1), dtype=torch.uint8),) + planes(4, 8)[1:],
    "four planes": planes(4, 8) + (planes(4, 8)[1],),
    "not a tensor": (planes(4, 8)[0], None),
    "y stride": (torch.zeros((4, 16), dtype=torch.uint8)[:, ::2],) + planes(4, 8)[1:],
    "u stride": (planes(4, 8)[0], torch.zeros((2, 8), dtype=torch.uint8)[:, ::2], planes(4, 8)[2]),
    "uv stride": (planes(4, 8)[0], torch.zeros((2, 4, 4), dtype=torch.uint8)[..., ::2]),
    "single stride": torch.zeros((6, 16), dtype=torch.uint8)[:, ::2],
    "pitches differ": (planes(4, 8)[0], torch.zeros((2, 6), dtype=torch.uint8)[:, :4], planes(4, 8)[2]),
    "mixed devices in a frame": (planes(4, 8)[0], planes(4, 8, device="meta")[1], planes(4, 8)[2]),
}


@pytest.mark.parametrize("what", sorted(BAD_FRAMES))
def test_malformed_frames_raise_value_error(what):
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    bad = BAD_FRAMES[what]
    calls = [lambda: cl.letterbox_yuv420([bad], 32, 32), lambda: cl.tile_yuv420([bad], 32, 32),
             lambda: cl.letterbox_yuv420([planes(4, 8), bad], 32, 32, layout="i420"),
             lambda: model.detect_frames([bad], 32, 32, pixel_format="nv12"), lambda: model.detect_tiled([bad], tile=(32, 32), pixel_format="i420")]
    for call in calls:
        with pytest.raises(ValueError):
            call()


def test_unknown_options_empty_batches_and_cpu_frames_are_refused():
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    good = planes(4, 8)
    for kw in ({"layout": "yv12"}, {"layout": "rgb"}, {"matrix": "bt2020"}, {"matrix": None}):
        with pytest.raises(ValueError):
            cl.letterbox_yuv420([good], 32, 32, **kw)
        with pytest.raises(ValueError):
            cl.tile_yuv420([good], 32, 32, **kw)
    for kw in ({"pixel_format": "yv12"}, {"pixel_format": "nv12", "matrix": "bt2020"}, {"pixel_format": "i420", "matrix": "rec709"}):
        with pytest.raises(ValueError):
            model.detect_frames([good], 32, 32, **kw)
        with pytest.raises(ValueError):
            model.detect_tiled([good], tile=(32, 32), **kw)
    with pytest.raises(ValueError):
        cl.yuv_coefficients("bt2020")
    with pytest.raises(ValueError):
        cl.letterbox_yuv420([], 32, 32)
    with pytest.raises(ValueError):
        cl.tile_yuv420([], 32, 32)
    with pytest.raises(ValueError):
        cl.letterbox_yuv420(torch.zeros((6, 8), dtype=torch.uint8), 32, 32)           # a tensor must be [N, h*3/2, w]
    with pytest.raises(ValueError):
        cl.letterbox_yuv420([good], 500, 512)                                         # the canvas rule of letterbox_geometry
    with pytest.raises(ValueError):
        cl.letterbox_yuv420([good], 32, 32, fill=(0, 0, 256))
    # well-formed frames in host memory: no CPU fallback
    single = torch.zeros((6, 8), dtype=torch.uint8)
    for frames in ([good], [single], single[None], [(good[0], torch.stack(good[1:], dim=-1))]):
        with pytest.raises(RuntimeError, match="HIP devices only"):
            cl.letterbox_yuv420(frames, 32, 32)
        with pytest.raises(RuntimeError, match="HIP devices only"):
            cl.tile_yuv420(frames, 32, 32, layout="i420")
        with pytest.raises(RuntimeError, match="HIP devices only"):
            model.letterbox_yuv420(frames, 32, 32)
        with pytest.raises(RuntimeError):
            model.detect_frames(frames, 32, 32, pixel_format="nv12")
        with pytest.raises(RuntimeError):
            model.detect_tiled(frames, tile=(32, 32), pixel_format="i420")
    with pytest.raises(RuntimeError):
        model.detect_frames(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))            # "rgb" is still today's path


# ----------------------------------------------------------------------------- geometry
def test_geometry_is_letterbox_geometry_and_tile_grid_of_the_frame_size(monkeypatch):
    """The records the kernel would read, captured at the launch (no device: the launch is replaced)."""
    seen = {}

    class Captured(Exception):
        pass

    def fake_gather(dev, windows, plain, height, width, C, word, planes=None, coef=None, merge_records=None, frame_first_view=None):
        seen.update(windows=windows, size=(height, width), coef=coef, word=word, C=C)
        raise Captured

    monkeypatch.setattr(_gather, "gather", fake_gather)                 # the one launch path of the YUV and the packed functions
    monkeypatch.setattr(_gather, "require_hip", lambda tensors, what: None)
    sizes = [(1080, 1920), (720, 1280), (1280, 720), (2, 2), (16, 8), (34, 1000), (1000, 34), (1000, 1500)]
    frames = [planes(h, w) for (h, w) in sizes]
    for (height, width) in ((512, 512), (608, 1088)):
        with pytest.raises(Captured):
            cl.letterbox_yuv420(frames, height, width, matrix="bt709", fill=(1, 2, 3))
        assert seen["size"] == (height, width) and seen["coef"] == cl.yuv_coefficients("bt709") and seen["word"] == 0x030201
        for n, (h, w) in enumerate(sizes):
            g = cl.letterbox_geometry(h, w, height, width)
            assert g == letterbox_ref.geometry(h, w, height, width)
            assert seen["windows"][n] == (n, 0, 0, h, w) + g
    with pytest.raises(Captured):
        cl.tile_yuv420(frames, 512, 512, 0.1, True)
    rec, ffv, views = tiled_ref.view_records(sizes, 512, 512, 0.1, True, letterbox_ref.geometry)
    assert [(n, y0, x0, h, w) for (n, y0, x0, h, w, *_) in seen["windows"]] == views
    i = 0
    for n, (h, w) in enumerate(sizes):
        for (y0, x0, th, tw) in cl.tile_grid(h, w, 512, 512, 0.1):
            assert seen["windows"][i] == (n, y0, x0, th, tw, th, tw, 0, 0)
            i += 1
        assert seen["windows"][i] == (n, 0, 0, h, w) + cl.letterbox_geometry(h, w, 512, 512)
        i += 1
        assert i == ffv[n + 1]
    assert any(x0 % 2 or y0 % 2 for (_, y0, x0, *_) in seen["windows"])            # odd origins occur: overlap 0.1 of 512 is a step of 461
    # letterbox_uint8 / tile_uint8 hand the same launch path the same windows
    yuv_tile_windows = seen["windows"]
    rgb = [torch.zeros((h, w, 3), dtype=torch.uint8) for (h, w) in sizes]
    for (height, width) in ((512, 512), (608, 1088)):
        with pytest.raises(Captured):
            cl.letterbox.letterbox_uint8(rgb, height, width, fill=(1, 2, 3))
        assert seen["size"] == (height, width) and seen["coef"] is None and seen["word"] == 0x030201 and seen["C"] == 3
        assert seen["windows"] == [(n, 0, 0, h, w) + cl.letterbox_geometry(h, w, height, width) for n, (h, w) in enumerate(sizes)]
    with pytest.raises(Captured):
        cl.tile_uint8(rgb, 512, 512, 0.1, True)
    assert seen["size"] == (512, 512) and seen["coef"] is None and seen["windows"] == yuv_tile_windows


# ----------------------------------------------------------------------------- the C ABI
def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", header), f"{ENTRY} is not declared in include/centernet_gfx950.h"
    assert ENTRY in _lib.EXPORTED_SYMBOLS and hasattr(lib, ENTRY)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # an entry point and a record struct only: no ABI bump
    assert "cnl_yuv420_frame" in header and ctypes.sizeof(_lib.Yuv420Frame) == 72
    assert [(n, getattr(_lib.Yuv420Frame, n).offset) for n, _ in _lib.Yuv420Frame._fields_] == [
        ("y", 0), ("u", 8), ("v", 16), ("y_pitch", 24), ("c_pitch", 28), ("c_step", 32), ("x0", 36), ("y0", 40), ("h", 44), ("w", 48),
        ("new_h", 52), ("new_w", 56), ("pad_top", 60), ("pad_left", 64), ("reserved", 68)]
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        assert ENTRY in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ("letterbox_yuv420", "tile_yuv420", "yuv_coefficients", "split_planes"):
        assert callable(getattr(cl, name)) and name in cl.__all__


def test_entry_point_validates_arguments_without_a_device():
    lib = _lib.load()
    E, U = _lib.CNL_E_BAD_ARG, _lib.CNL_E_UNSUPPORTED
    fake = 0x10000          # never dereferenced: every call below fails validation first
    coef = (ctypes.c_int32 * 6)(*cl.yuv_coefficients())
    f = getattr(lib, ENTRY)
    assert f(fake, fake, -1, 512, 512, coef, 0, None) == E and "N = -1" in _lib.last_error()
    assert f(fake, fake, 65536, 512, 512, coef, 0, None) == E
    assert f(None, fake, 1, 512, 512, coef, 0, None) == E and "null" in _lib.last_error()
    assert f(fake, None, 1, 512, 512, coef, 0, None) == E
    assert f(fake, fake, 1, 512, 512, None, 0, None) == E and "null" in _lib.last_error()
    assert f(fake, fake, 1, 500, 512, coef, 0, None) == E and "multiple of 32" in _lib.last_error()
    assert f(fake, fake, 1, 512, 0, coef, 0, None) == E
    assert f(fake + 4, fake, 1, 512, 512, coef, 0, None) == E and "aligned" in _lib.last_error()
    assert f(fake, fake + 2, 1, 512, 512, coef, 0, None) == E and "aligned" in _lib.last_error()
    for bad in ((16, 1 << 24, 0, 0, 0, 0), (16, 1220542, 1 << 24, 0, 0, 0), (16, 1220542, 0, -(1 << 23), -(1 << 23), 0), (16, 1220542, 0, 0, 0, -(1 << 24)),
                (-1, 1220542, 0, 0, 0, 0), (256, 1220542, 0, 0, 0, 0), (16, -1, 0, 0, 0, 0)):
        assert f(fake, fake, 1, 512, 512, (ctypes.c_int32 * 6)(*bad), 0, None) == U and "overflow" in _lib.last_error(), bad
    # two faults at once: N, the canvas, the coefficients (of an empty batch too), then the pointers — in that order
    over = (ctypes.c_int32 * 6)(16, 1 << 24, 0, 0, 0, 0)
    assert f(fake, fake, -1, 500, 512, None, 0, None) == E and "N = -1" in _lib.last_error()
    assert f(fake, fake, 1, 500, 512, None, 0, None) == E and "multiple of 32" in _lib.last_error()
    assert f(fake, fake, 1, 500, 512, over, 0, None) == E and "multiple of 32" in _lib.last_error()
    assert f(None, fake + 2, 1, 512, 512, None, 0, None) == E and "null coefficients" in _lib.last_error()
    assert f(None, None, 1, 512, 512, over, 0, None) == U and "overflow" in _lib.last_error()
    assert f(None, None, 0, 512, 512, over, 0, None) == U and f(None, None, 0, 512, 512, None, 0, None) == E
    assert f(None, fake + 2, 1, 512, 512, coef, 0, None) == E and "null pointer" in _lib.last_error()
    assert f(None, None, 0, 512, 512, coef, 0, None) == 0           # an empty batch is a no-op
    for matrix, full_range in COMBOS:                               # every set the host can choose passes the overflow condition
        assert f(None, None, 0, 512, 512, (ctypes.c_int32 * 6)(*cl.yuv_coefficients(matrix, full_range)), 0, None) == 0
    with pytest.raises(ValueError):
        _lib.check(U, "x")
