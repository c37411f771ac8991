"""No GPU: the crop window / live / target rules (tests/crop_ref.py) on hand-worked cases, the record packing crop_detections shares with
the gather path, the refusals of the Python surface, and cnl_crop_boxes_u8's declaration and argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import crop_ref
import letterbox_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _gather, _lib, crops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cnl_crop_boxes_u8"
H, W = 50, 100                                   # the frame of the known answers: 100 pixels wide, 50 high


# ----------------------------------------------------------------------------- the window rule, worked by hand
def test_window_known_answers():
    # floor(10.2) = 10, ceil(20.0) = 20; floor(5.0) = 5, ceil(9.5) = 10
    assert crop_ref.window((10.2, 5.0, 20.0, 9.5), H, W) == (10, 5, 10, 5)
    # pad 0.1: bw = 9.8 -> 0.98, bh = 4.5 -> 0.45: floor(9.22) = 9, ceil(20.98) = 21; floor(4.55) = 4, ceil(9.95) = 10
    assert crop_ref.window((10.2, 5.0, 20.0, 9.5), H, W, pad=0.1) == (9, 4, 12, 6)
    # over the right / bottom edge: clipped to W = 100, H = 50
    assert crop_ref.window((90.5, 40.5, 120.0, 70.0), H, W) == (90, 40, 10, 10)
    # over the left / top edge, and a pad that pushes the window past every edge: the whole frame
    assert crop_ref.window((-7.5, -2.0, 3.2, 4.0), H, W) == (0, 0, 4, 4)
    assert crop_ref.window((10.0, 5.0, 90.0, 45.0), H, W, pad=1.0) == (0, 0, W, H)
    assert crop_ref.window((0.0, 0.0, 100.0, 50.0), H, W) == (0, 0, W, H)


def test_dead_windows():
    assert crop_ref.window((110.0, 10.0, 130.0, 20.0), H, W) is None              # wholly outside, right: x0 = xe = 100
    assert crop_ref.window((-30.0, -30.0, -5.0, -5.0), H, W) is None              # wholly outside, top left: x0 = xe = 0
    assert crop_ref.window((10.0, 60.0, 20.0, 70.0), H, W) is None                # below
    assert crop_ref.window((20.0, 5.0, 10.0, 9.0), H, W) is None                  # inverted in x: w = 10 - 20
    assert crop_ref.window((10.0, 9.0, 20.0, 5.0), H, W) is None                  # inverted in y
    assert crop_ref.window((10.0, 5.0, 10.0, 9.0), H, W) is None                  # x1 == x2 on an integer: floor = ceil
    assert crop_ref.window((10.5, 5.0, 10.5, 9.0), H, W) == (10, 5, 1, 4)         # ... off an integer: one column
    assert crop_ref.window((10.0, 5.5, 20.0, 5.5), H, W) == (10, 5, 10, 1)
    assert crop_ref.window((10.2, 5.0, 20.0, 9.5), H, W, live=False) is None
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in range(4):
            box = [10.2, 5.0, 20.0, 9.5]
            box[i] = bad
            assert crop_ref.window(box, H, W) is None and crop_ref.window(box, H, W, pad=0.25) is None


def test_huge_magnitudes_do_not_overflow_the_integer_conversion():
    assert crop_ref.window((-1e30, -1e30, 1e30, 1e30), H, W) == (0, 0, W, H)
    assert crop_ref.window((-1e30, -1e30, 1e30, 1e30), H, W, pad=0.5) == (0, 0, W, H)
    assert crop_ref.window((-1e30, 5.0, 20.0, 9.5), H, W) == (0, 5, 20, 5)
    assert crop_ref.window((10.2, 5.0, 1e30, 1e30), H, W, pad=1e10) == (0, 0, W, H)      # pad * bw overflows to inf: still clamped
    assert crop_ref.window((1e30, 5.0, 2e30, 9.0), H, W) is None
    assert crop_ref.window((-2e30, 5.0, -1e30, 9.0), H, W) is None


def test_live_rule():
    assert crop_ref.is_live(3) and crop_ref.is_live(3, n_count=4) and not crop_ref.is_live(4, n_count=4)
    assert crop_ref.is_live(0, score=0.5, threshold=0.5) and not crop_ref.is_live(0, score=0.49, threshold=0.5)
    assert not crop_ref.is_live(0, score=float("nan"), threshold=0.0)
    assert not crop_ref.is_live(5, n_count=4, score=0.9, threshold=0.5) and not crop_ref.is_live(1, n_count=4, score=0.1, threshold=0.5)
    assert crop_ref.is_live(1, n_count=4, score=0.9, threshold=0.5)
    # the threshold is compared in float32, as the library's float argument is
    assert crop_ref.is_live(0, score=np.float32(0.3), threshold=0.3)


def test_keep_aspect_geometry_is_the_letterbox_rule():
    for (ch, cw) in ((128, 64), (64, 128), (32, 32), (20, 12), (1, 4), (112, 112)):
        for h in list(range(1, 70)) + [100, 255, 256, 257, 719, 1080]:
            for w in (1, 2, 3, 5, 8, 13, 31, 64, 65, 127, 640, 1920):
                g = crop_ref.geometry(h, w, ch, cw, True)
                assert g == letterbox_ref.geometry(h, w, ch, cw), (h, w, ch, cw)
                assert 1 <= g[0] <= ch and 1 <= g[1] <= cw and g[2] + g[0] <= ch and g[3] + g[1] <= cw
                assert crop_ref.geometry(h, w, ch, cw, False) == (ch, cw, 0, 0)
    for (h, w) in ((64, 64), (128, 128), (720, 720)):          # a multiple-of-32 target: the package's own function agrees
        assert crop_ref.geometry(h, w, 128, 64, True) == cl.letterbox_geometry(h, w, 128, 64)


# ----------------------------------------------------------------------------- record packing, shared with the gather path
def test_record_packing_fills_the_two_structs():
    windows = [(0, 0, 0, 1080, 1920, 288, 512, 112, 0), (1, 3, 5, 7, 9, 11, 13, 15, 17)]
    plain = [(0x7f0000001000, 5760), (0x7f0000002008, 100)]
    rec = np.zeros((2, 5), dtype=np.int64)
    _gather.pack_plain(rec, windows, plain)
    got = (_lib.LetterboxFrame * 2).from_buffer_copy(rec.tobytes())
    for g, (_, _, _, h, w, nh, nw, pt, pl), (addr, stride) in zip(got, windows, plain):
        assert (g.src, g.h, g.w, g.row_stride, g.new_h, g.new_w, g.pad_top, g.pad_left, g.reserved) == (addr, h, w, stride, nh, nw, pt, pl, 0)
    planes = [(0x7f0000003000, 0x7f0000004000, 0x7f0000004001, 2048, 2048, 2), (0x10, 0x20, 0x30, 64, 32, 1)]
    rec = np.zeros((2, 9), dtype=np.int64)
    _gather.pack_yuv(rec, windows, planes)
    got = (_lib.Yuv420Frame * 2).from_buffer_copy(rec.tobytes())
    for g, (_, y0, x0, h, w, nh, nw, pt, pl), p in zip(got, windows, planes):
        assert (g.y, g.u, g.v, g.y_pitch, g.c_pitch, g.c_step) == p
        assert (g.x0, g.y0, g.h, g.w, g.new_h, g.new_w, g.pad_top, g.pad_left, g.reserved) == (x0, y0, h, w, nh, nw, pt, pl, 0)


# ----------------------------------------------------------------------------- the Python surface
def yuv_planes(h, w, device="cpu"):
    return (torch.zeros((h, w), dtype=torch.uint8, device=device), torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=device),
            torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=device))


def test_cpu_tensors_are_refused():
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    frames = [torch.zeros((8, 8, 3), dtype=torch.uint8)]
    boxes = torch.zeros((1, 2, 4))
    for f in (cl.crop_detections, crops.crop_detections, model.crop_detections):
        with pytest.raises(RuntimeError, match="HIP devices only"):
            f(frames, boxes)
        with pytest.raises(RuntimeError, match="HIP devices only"):
            f(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), boxes)
        with pytest.raises(RuntimeError, match="HIP devices only"):
            f([yuv_planes(4, 8)], boxes, pixel_format="nv12")
        with pytest.raises(RuntimeError, match="HIP devices only"):
            f([torch.zeros((6, 8), dtype=torch.uint8)], boxes, pixel_format="i420")


def test_malformed_arguments_raise_value_error(monkeypatch):
    """With the device check switched off, every refusal below fires before anything is launched."""
    monkeypatch.setattr(_gather, "require_hip", lambda tensors, what: None)
    frames = [torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((6, 10, 3), dtype=torch.uint8)]
    boxes = torch.zeros((2, 3, 4))
    scores, count = torch.zeros((2, 3)), torch.zeros((2,), dtype=torch.int32)
    bad_calls = {
        "width % 4": lambda: cl.crop_detections(frames, boxes, size=(128, 62)),
        "width 0": lambda: cl.crop_detections(frames, boxes, size=(128, 0)),
        "height 0": lambda: cl.crop_detections(frames, boxes, size=(0, 64)),
        "size not a pair": lambda: cl.crop_detections(frames, boxes, size=128),
        "size float": lambda: cl.crop_detections(frames, boxes, size=(128.0, 64)),
        "boxes dtype": lambda: cl.crop_detections(frames, boxes.double()),
        "boxes shape": lambda: cl.crop_detections(frames, torch.zeros((2, 3, 5))),
        "boxes 2-d": lambda: cl.crop_detections(frames, torch.zeros((2, 4))),
        "boxes not contiguous": lambda: cl.crop_detections(frames, torch.zeros((2, 3, 8))[..., ::2]),
        "boxes not a tensor": lambda: cl.crop_detections(frames, boxes.numpy()),
        "N mismatch": lambda: cl.crop_detections(frames, torch.zeros((3, 3, 4))),
        "boxes on another device": lambda: cl.crop_detections(frames, torch.zeros((2, 3, 4), device="meta")),
        "frames on different devices": lambda: cl.crop_detections([frames[0], torch.zeros((8, 8, 3), dtype=torch.uint8, device="meta")], boxes),
        "frames dtype": lambda: cl.crop_detections([f.float() for f in frames], boxes),
        "frames mixed C": lambda: cl.crop_detections([frames[0], torch.zeros((8, 8, 4), dtype=torch.uint8)], boxes),
        "frames C = 5": lambda: cl.crop_detections([torch.zeros((8, 8, 5), dtype=torch.uint8)] * 2, boxes),
        "no frames": lambda: cl.crop_detections([], boxes),
        "tensor not 4-d": lambda: cl.crop_detections(torch.zeros((8, 8, 3), dtype=torch.uint8), boxes),
        "scores without threshold": lambda: cl.crop_detections(frames, boxes, scores=scores),
        "threshold without scores": lambda: cl.crop_detections(frames, boxes, score_threshold=0.3),
        "threshold NaN": lambda: cl.crop_detections(frames, boxes, scores=scores, score_threshold=float("nan")),
        "scores shape": lambda: cl.crop_detections(frames, boxes, scores=torch.zeros((2, 4)), score_threshold=0.3),
        "scores dtype": lambda: cl.crop_detections(frames, boxes, scores=scores.double(), score_threshold=0.3),
        "scores device": lambda: cl.crop_detections(frames, boxes, scores=torch.zeros((2, 3), device="meta"), score_threshold=0.3),
        "count dtype": lambda: cl.crop_detections(frames, boxes, count=count.long()),
        "count shape": lambda: cl.crop_detections(frames, boxes, count=torch.zeros((3,), dtype=torch.int32)),
        "pad negative": lambda: cl.crop_detections(frames, boxes, pad=-0.1),
        "pad NaN": lambda: cl.crop_detections(frames, boxes, pad=float("nan")),
        "pad inf": lambda: cl.crop_detections(frames, boxes, pad=float("inf")),
        "fill": lambda: cl.crop_detections(frames, boxes, fill=(0, 0, 256)),
        "pixel format": lambda: cl.crop_detections(frames, boxes, pixel_format="yv12"),
        "matrix": lambda: cl.crop_detections([yuv_planes(4, 8)] * 2, boxes, pixel_format="nv12", matrix="bt2020"),
        "C != 3 with a YUV format": lambda: cl.crop_detections([torch.zeros((8, 8, 4), dtype=torch.uint8)] * 2, boxes, pixel_format="nv12"),
        "packed RGB with a YUV format": lambda: cl.crop_detections(frames, boxes, pixel_format="i420"),
        "odd YUV frame": lambda: cl.crop_detections([torch.zeros((9, 7), dtype=torch.uint8)] * 2, boxes, pixel_format="nv12"),
        "YUV N mismatch": lambda: cl.crop_detections([yuv_planes(4, 8)], boxes, pixel_format="i420"),
    }
    for what, call in bad_calls.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{what}: not refused")


# ----------------------------------------------------------------------------- the C ABI
def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", header), f"{ENTRY} is not declared in include/centernet_gfx950.h"
    assert ENTRY in _lib.EXPORTED_SYMBOLS and hasattr(lib, ENTRY)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # an entry point only: no ABI bump
    for phrase in ("Live rule", "Window rule", "floorf(xa)", "ceilf(xb)"):
        assert phrase in header, phrase
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        assert ENTRY in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert callable(cl.crop_detections) and "crop_detections" in cl.__all__ and callable(cl.CenterNet.crop_detections)


def call(lib, frames=0x10000, boxes=0x20000, scores=None, threshold=0.0, count=None, N=1, k=2, C=3, coef=None, pad=0.0, keep=0,
         records=0x30000, windows=0x40000, out=0x50000, ch=128, cw=64):
    """The entry with fake pointers (never dereferenced: every call made with them fails validation or is a no-op)."""
    return getattr(lib, ENTRY)(frames, boxes, scores, threshold, count, N, k, C, coef, pad, keep, records, windows, out, ch, cw, 0, None)


def test_entry_point_validates_arguments_without_a_device():
    lib = _lib.load()
    E, U = _lib.CNL_E_BAD_ARG, _lib.CNL_E_UNSUPPORTED
    coef = (ctypes.c_int32 * 6)(*cl.yuv_coefficients())
    assert call(lib, N=-1) == E and "negative N or k" in _lib.last_error()
    assert call(lib, k=-1) == E and "negative N or k" in _lib.last_error()
    assert call(lib, N=65536, k=65536) == E and "slots" in _lib.last_error()
    for C in (0, 5, -3):
        assert call(lib, C=C) == E and f"C = {C}" in _lib.last_error()
    for C in (1, 2, 4):
        assert call(lib, C=C, coef=coef) == E and "YUV" in _lib.last_error()
    for (ch, cw) in ((128, 62), (128, 66), (128, 0), (128, -4), (128, 2), (0, 64), (-1, 64)):
        assert call(lib, ch=ch, cw=cw) == E and "multiple of 4" in _lib.last_error(), (ch, cw)
    assert call(lib, ch=1 << 20, cw=1 << 20) == E and "2 GiB" in _lib.last_error()
    for pad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(lib, pad=pad) == E and "pad" in _lib.last_error()
    assert call(lib, scores=0x60000, threshold=float("nan")) == E and "score_threshold" in _lib.last_error()
    for bad in ((16, 1 << 24, 0, 0, 0, 0), (16, 1220542, 1 << 24, 0, 0, 0), (-1, 1220542, 0, 0, 0, 0), (256, 1220542, 0, 0, 0, 0), (16, -1, 0, 0, 0, 0)):
        assert call(lib, coef=(ctypes.c_int32 * 6)(*bad)) == U and "overflow" in _lib.last_error() and ENTRY in _lib.last_error(), bad
        assert call(lib, coef=(ctypes.c_int32 * 6)(*bad), N=0) == U                      # of an empty batch too, as the sibling entry
    for name in ("frames", "boxes", "records", "windows", "out"):
        assert call(lib, **{name: None}) == E and "null pointer" in _lib.last_error(), name
    for name, off in (("frames", 4), ("records", 4), ("boxes", 8), ("windows", 8), ("out", 2), ("scores", 2), ("count", 2)):
        base = {"frames": 0x10000, "boxes": 0x20000, "records": 0x30000, "windows": 0x40000, "out": 0x50000, "scores": 0x60000, "count": 0x70000}
        assert call(lib, **{name: base[name] + off}) == E and "aligned" in _lib.last_error(), name
    # no slots: a no-op whose pointers are not looked at, for packed and YUV frames
    for kw in ({"N": 0}, {"k": 0}, {"N": 0, "k": 0}):
        assert call(lib, frames=None, boxes=None, records=None, windows=None, out=None, **kw) == 0
        assert call(lib, frames=None, boxes=None, records=None, windows=None, out=None, coef=coef, **kw) == 0
    for (ch, cw) in ((112, 112), (224, 224), (256, 128), (128, 64), (1, 4), (20, 12)):   # the crop canvas rule is not the network's
        assert call(lib, N=0, ch=ch, cw=cw) == 0
    # the sibling entry still reports its coefficients under its own name (the check is shared)
    f = lib.cnl_letterbox_yuv420_u8
    assert f(None, None, 0, 512, 512, (ctypes.c_int32 * 6)(16, 1 << 24, 0, 0, 0, 0), 0, None) == U
    assert "cnl_letterbox_yuv420_u8" in _lib.last_error() and "overflow" in _lib.last_error()
    assert f(None, None, 0, 512, 512, None, 0, None) == E and "cnl_letterbox_yuv420_u8: null coefficients" in _lib.last_error()
