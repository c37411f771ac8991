"""No GPU: cnl_draw_boxes_u8's declaration, yuv.rgb_to_yuv's known answers, the overlay rule (tests/overlay_ref.py) on hand-written
cases, the refusals of the Python surface and the entry point's argument checks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import overlay_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _gather, _lib, overlay, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cnl_draw_boxes_u8"
RED, WHITE = (200, 10, 20), (255, 255, 255)


# ----------------------------------------------------------------------------- the C ABI
def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", header), f"{ENTRY} is not declared in include/centernet_gfx950.h"
    assert ENTRY in _lib.EXPORTED_SYMBOLS and hasattr(lib, ENTRY)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # an entry point only: no ABI bump
    for phrase in ("Live rule", "Corners", "rintf(x)", "Ring", "SQUARE corners", "Order", "01110 10001 10011 10101 11001 10001 01110"):
        assert phrase in header, phrase
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        assert ENTRY in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert callable(cl.draw_detections) and "draw_detections" in cl.__all__ and callable(cl.CenterNet.draw_detections)
    assert "rgb_to_yuv" in cl.__all__ and "DEFAULT_PALETTE" in cl.__all__


def test_header_glyphs_are_the_references():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    for d, rows in overlay_ref.GLYPH_ROWS.items():
        assert f"{d}: {rows}" in header, d


def call(lib, frames=0x10000, boxes=0x20000, labels=None, numbers=None, scores=None, threshold=0.0, count=None, N=1, k=2, C=3, yuv=0,
         palette=0x30000, P=4, thickness=2, alpha=0, scale=2, max_h=64, max_w=64, records=0x40000):
    """The entry with fake pointers (never dereferenced: every call made with them fails validation or is a no-op)."""
    return getattr(lib, ENTRY)(frames, boxes, labels, numbers, scores, threshold, count, N, k, C, yuv, palette, P, thickness, alpha, scale,
                               max_h, max_w, records, None)


def test_entry_point_validates_arguments_without_a_device():
    lib = _lib.load()
    E = _lib.CNL_E_BAD_ARG
    assert call(lib, N=-1) == E and "negative N or k" in _lib.last_error()
    assert call(lib, k=-1) == E and "negative N or k" in _lib.last_error()
    assert call(lib, N=65536) == E and "65535" in _lib.last_error()
    assert call(lib, N=65535, k=65536) == E and "slots" in _lib.last_error()
    for C in (0, 1, 2, 5):
        assert call(lib, C=C) == E and f"C = {C}" in _lib.last_error()
    assert call(lib, C=4, yuv=1) == E and "C = 4" in _lib.last_error()
    for kw, word in (({"P": 0}, "palette"), ({"P": 257}, "palette"), ({"thickness": 0}, "thickness"), ({"thickness": 33}, "thickness"),
                     ({"alpha": -1}, "fill_alpha"), ({"alpha": 257}, "fill_alpha"), ({"scale": -1}, "tag_scale"), ({"scale": 9}, "tag_scale"),
                     ({"max_h": 0}, "largest frame"), ({"max_w": 32769}, "largest frame")):
        assert call(lib, **kw) == E and word in _lib.last_error(), kw
    assert call(lib, scores=0x60000, threshold=float("nan")) == E and "score_threshold" in _lib.last_error()
    for name in ("frames", "boxes", "palette", "records"):
        assert call(lib, **{name: None}) == E and "null pointer" in _lib.last_error(), name
    base = {"frames": 0x10000, "boxes": 0x20000, "palette": 0x30000, "records": 0x40000, "labels": 0x50000, "numbers": 0x60000,
            "scores": 0x70000, "count": 0x80000}
    for name, off in (("frames", 4), ("labels", 4), ("boxes", 8), ("records", 8), ("palette", 2), ("numbers", 2), ("scores", 2), ("count", 2)):
        assert call(lib, **{name: base[name] + off}) == E and "aligned" in _lib.last_error(), name
    for kw in ({"N": 0}, {"k": 0}, {"N": 0, "k": 0}):             # no slots: a no-op whose pointers are not looked at
        assert call(lib, frames=None, boxes=None, palette=None, records=None, **kw) == 0
        assert call(lib, frames=None, boxes=None, palette=None, records=None, yuv=1, **kw) == 0


# ----------------------------------------------------------------------------- colours
def test_rgb_to_yuv_known_answers():
    assert yuv.rgb_to_yuv((255, 255, 255)) == (235, 128, 128)
    assert yuv.rgb_to_yuv((0, 0, 0)) == (16, 128, 128)
    assert yuv.rgb_to_yuv((255, 0, 0)) == (81, 90, 240)
    assert yuv.rgb_to_yuv((255, 255, 255), "bt601", True) == (255, 128, 128)
    assert cl.rgb_to_yuv is yuv.rgb_to_yuv
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            lo, hi = (0, 255) if full else (16, 235)
            assert yuv.rgb_to_yuv((255, 255, 255), matrix, full) == (hi, 128, 128)
            assert yuv.rgb_to_yuv((0, 0, 0), matrix, full) == (lo, 128, 128)
            assert yuv.rgb_to_yuv((128, 128, 128), matrix, full)[1:] == (128, 128)             # greys carry no chroma
            # pure red and blue sit at the top of Cr / Cb: 128 + 112 = 240 limited; 128 + 127.5 = 255.5, half to even 256, clamped, full
            assert yuv.rgb_to_yuv((255, 0, 0), matrix, full)[2] == (255 if full else 240)
            assert yuv.rgb_to_yuv((0, 0, 255), matrix, full)[1] == (255 if full else 240)
    # bt709 limited red, by hand: Y = 16 + 219 * 0.2126 = 62.56 -> 63; Cb = 128 - 224 * 0.2126 / 1.8556 = 102.34 -> 102
    assert yuv.rgb_to_yuv((255, 0, 0), "bt709") == (63, 102, 240)
    # bt601 full-range red: Y = 76.245 -> 76; Cb = 128 - 76.245 / 1.772 = 84.97 -> 85
    assert yuv.rgb_to_yuv((255, 0, 0), "bt601", True) == (76, 85, 255)
    for bad in ((256, 0, 0), (0, -1, 0), (1, 2), "red"):
        with pytest.raises(ValueError):
            yuv.rgb_to_yuv(bad)
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv((1, 2, 3), "bt2020")


def test_default_palette():
    pal = overlay.DEFAULT_PALETTE
    assert cl.DEFAULT_PALETTE is pal and len(pal) >= 16 and len(set(pal)) == len(pal)
    assert all(len(c) == 3 and all(isinstance(v, int) and 0 <= v <= 255 for v in c) for c in pal)


# ----------------------------------------------------------------------------- the rule, worked by hand
def test_corners_round_half_to_even_and_clamp():
    assert overlay_ref.corners((0.5, 1.5, 2.5, 3.5)) == (0, 2, 2, 4)
    assert overlay_ref.corners((-0.5, -1.5, 10.49, 10.51)) == (0, -2, 10, 11)
    assert overlay_ref.corners((-1e30, -1e30, 1e30, 1e30)) == (-32768, -32768, 32767, 32767)
    assert overlay_ref.corners((3.4, 0.0, 2.6, 5.0)) == (3, 0, 3, 5)                 # rounds to X1 == X2: a live one-column box
    assert overlay_ref.corners((4.0, 0.0, 2.0, 5.0)) is None and overlay_ref.corners((0.0, 4.0, 5.0, 2.0)) is None
    assert overlay_ref.corners((1.0, 1.0, 5.0, 5.0), live=False) is None
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in range(4):
            box = [1.0, 1.0, 5.0, 5.0]
            box[i] = bad
            assert overlay_ref.corners(box) is None
    assert overlay_ref.is_live(3, n_count=4) and not overlay_ref.is_live(4, n_count=4)
    assert overlay_ref.is_live(0, score=np.float32(0.3), threshold=0.3) and not overlay_ref.is_live(0, score=float("nan"), threshold=0.0)


def draw_one(h, w, box, **kw):
    frame = np.zeros((h, w, 3), dtype=np.uint8)
    numbers = kw.pop("numbers", None)
    return overlay_ref.draw_reference([frame], np.float32([[box]]), [RED], WHITE, numbers=None if numbers is None else [[numbers]], **kw)[0]


def test_thickness_1_ring_is_exactly_the_outline():
    out = draw_one(8, 8, (2.0, 1.0, 5.0, 6.0), thickness=1, tag_scale=0)
    want = np.zeros((8, 8), dtype=bool)
    want[1, 2:6] = want[6, 2:6] = True
    want[1:7, 2] = want[1:7, 5] = True
    assert np.array_equal((out == RED).all(-1), want) and (out[~want] == 0).all() and want.sum() == 16


def test_ring_extent_for_thickness_2_and_5():
    # t = 2: o = 0, i = 2 -> columns X1, X1 + 1 and X2 - 1, X2 (the ring grows inwards)
    out = draw_one(20, 20, (5.0, 6.0, 14.0, 15.0), thickness=2, tag_scale=0)
    ring = (out == RED).all(-1)
    assert not ring[6:16, 5:15].all() and ring[6:8, 5:15].all() and ring[14:16, 5:15].all() and ring[6:16, 5:7].all() and ring[6:16, 13:15].all()
    assert not ring[8:14, 7:13].any() and ring.sum() == 10 * 10 - 6 * 6
    assert not ring[5].any() and not ring[16].any() and not ring[:, 4].any() and not ring[:, 15].any()
    # t = 5: o = 2, i = 3 -> from X1 - 2 to X1 + 2: five pixels centred on the corner
    out = draw_one(24, 24, (6.0, 7.0, 16.0, 17.0), thickness=5, tag_scale=0)
    ring = (out == RED).all(-1)
    assert ring[5:20, 4:9].all() and ring[5:20, 14:19].all() and ring[5:10, 4:19].all() and ring[15:20, 4:19].all()
    assert not ring[10:15, 9:14].any() and ring.sum() == 15 * 15 - 5 * 5
    assert not ring[4].any() and not ring[20].any() and not ring[:, 3].any() and not ring[:, 19].any()
    # a box too small to have an inside is solid
    out = draw_one(12, 12, (4.0, 4.0, 6.0, 6.0), thickness=5, tag_scale=0)
    assert (out == RED).all(-1)[2:9, 2:9].all() and (out == RED).all(-1).sum() == 49


def test_tag_of_the_digit_1_at_scale_1():
    assert np.array_equal(overlay_ref.tag_bitmap(1, 1).astype(int), np.array([
        [0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 1, 0, 0, 0],
        [0, 0, 1, 1, 0, 0, 0],
        [0, 0, 0, 1, 0, 0, 0],
        [0, 0, 0, 1, 0, 0, 0],
        [0, 0, 0, 1, 0, 0, 0],
        [0, 0, 0, 1, 0, 0, 0],
        [0, 0, 1, 1, 1, 0, 0],
        [0, 0, 0, 0, 0, 0, 0]]))
    # on a frame: above the box, left edge at X1 (t = 1: o = 0), 7 wide and 9 high
    out = draw_one(30, 30, (10.0, 15.0, 25.0, 25.0), thickness=1, tag_scale=1, numbers=1)
    text = (out == WHITE).all(-1)
    assert np.array_equal(text[6:15, 10:17], overlay_ref.tag_bitmap(1, 1)) and text.sum() == 10
    assert ((out == RED).all(-1) | text)[6:15, 10:17].all() and (out[5, 10:17] == 0).all() and (out[6:15, 17] == 0).all()
    # two digits at scale 3: (6 * 2 + 1) * 3 = 39 wide, 27 high, every glyph pixel a 3 x 3 block
    bits = overlay_ref.tag_bitmap(40, 3)
    assert bits.shape == (27, 39) and np.array_equal(bits, np.kron(overlay_ref.tag_bitmap(40, 1), np.ones((3, 3), dtype=bool)))
    assert np.array_equal(overlay_ref.tag_bitmap(40, 1)[1:8, 1:6], overlay_ref.GLYPHS[4])
    assert np.array_equal(overlay_ref.tag_bitmap(40, 1)[1:8, 7:12], overlay_ref.GLYPHS[0])
    assert overlay_ref.tag_bitmap(1234567890, 1).shape == (9, 61)
    # no tag for a negative number or scale 0
    for kw in ({"numbers": -1, "tag_scale": 2}, {"numbers": 7, "tag_scale": 0}):
        assert not (draw_one(30, 30, (10.0, 15.0, 25.0, 25.0), thickness=1, **kw) == WHITE).all(-1).any()


def test_tag_moves_inside_the_box_when_there_is_no_room_above():
    out = draw_one(30, 30, (10.0, 8.0, 25.0, 25.0), thickness=1, tag_scale=1, numbers=1)          # T = 8 - 9 = -1 < 0 -> T = 8
    assert np.array_equal((out == WHITE).all(-1)[8:17, 10:17], overlay_ref.tag_bitmap(1, 1))
    assert not (out == WHITE).all(-1)[:8].any()
    out = draw_one(30, 30, (10.0, 9.0, 25.0, 25.0), thickness=1, tag_scale=1, numbers=1)          # T = 0: still above
    assert np.array_equal((out == WHITE).all(-1)[0:9, 10:17], overlay_ref.tag_bitmap(1, 1))
    out = draw_one(30, 30, (10.0, 10.0, 25.0, 25.0), thickness=5, tag_scale=1, numbers=1)         # o = 2: T = 10 - 2 - 9 = -1 -> 8, left 8
    assert np.array_equal((out == WHITE).all(-1)[8:17, 8:15], overlay_ref.tag_bitmap(1, 1))


def test_overlapping_fills_are_applied_from_the_last_slot_to_the_first():
    frame = np.full((10, 10, 3), 100, dtype=np.uint8)
    boxes = np.float32([[(0, 0, 6, 6), (3, 3, 9, 9)]])
    pal = [(200, 200, 200), (0, 0, 0)]
    out = overlay_ref.draw_reference([frame], boxes, pal, WHITE, labels=np.array([[0, 1]]), thickness=1, fill_alpha=128, tag_scale=0)[0]
    # slot 1 (black) first: (100 * 128 + 0 + 128) >> 8 = 50; then slot 0 (200): (50 * 128 + 200 * 128 + 128) >> 8 = 125
    assert (out[4, 4] == 125).all()
    # the reverse order would give (100 * 128 + 200 * 128 + 128) >> 8 = 150, then (150 * 128 + 128) >> 8 = 75
    assert (out[4, 4] != 75).all()
    assert (out[1, 1] == 150).all() and (out[8, 8] == 50).all()                     # each alone
    assert (out[0, 0] == 200).all() and (out[9, 9] == 0).all() and (out[6, 6] == 200).all()        # rings; slot 0's lies on top of slot 1's fill
    assert (out[3, 3] == 100).all()              # slot 1's black ring under slot 0's fill: (0 * 128 + 200 * 128 + 128) >> 8


def test_chroma_samples_are_painted_as_their_top_left_pixel():
    y, u, v = (np.zeros((8, 8), np.uint8), np.full((4, 4), 128, np.uint8), np.full((4, 4), 128, np.uint8))
    (yy, uu, vv), = overlay_ref.draw_reference_yuv([(y, u, v)], np.float32([[(1, 1, 5, 5)]]), [(81, 90, 240)], (235, 128, 128),
                                                   thickness=1, tag_scale=0)
    assert (yy[1, 1:6] == 81).all() and (yy[2:5, 2:5] == 0).all()
    # ring columns / rows 1 and 5 are odd: no chroma sample sits on them; with a solid fill samples (1..2, 1..2) = pixels 2 and 4 are in
    assert (uu == 128).all() and (vv == 128).all()
    (yy, uu, vv), = overlay_ref.draw_reference_yuv([(y, u, v)], np.float32([[(1, 1, 5, 5)]]), [(81, 90, 240)], (235, 128, 128),
                                                   thickness=1, tag_scale=0, fill_alpha=256)
    want = np.zeros((4, 4), dtype=bool)
    want[1:3, 1:3] = True
    assert np.array_equal(uu == 90, want) and np.array_equal(vv == 240, want) and (uu[~want] == 128).all()


# ----------------------------------------------------------------------------- the Python surface
def yuv_planes(h, w, device="cpu"):
    return (torch.zeros((h, w), dtype=torch.uint8, device=device), torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=device),
            torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=device))


def test_cpu_tensors_are_refused():
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    frames = [torch.zeros((8, 8, 3), dtype=torch.uint8)]
    boxes = torch.zeros((1, 2, 4))
    for f in (cl.draw_detections, overlay.draw_detections, model.draw_detections):
        for inplace in (False, True):
            with pytest.raises(RuntimeError, match="HIP devices only"):
                f(frames, boxes, inplace=inplace)
            with pytest.raises(RuntimeError, match="HIP devices only"):
                f(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), boxes, inplace=inplace)
            with pytest.raises(RuntimeError, match="HIP devices only"):
                f([yuv_planes(4, 8)], boxes, pixel_format="nv12", inplace=inplace)
            with pytest.raises(RuntimeError, match="HIP devices only"):
                f([torch.zeros((6, 8), dtype=torch.uint8)], boxes, pixel_format="i420", inplace=inplace)


def test_malformed_arguments_raise_value_error(monkeypatch):
    """With the device check switched off, every refusal below fires before anything is launched."""
    monkeypatch.setattr(_gather, "require_hip", lambda tensors, what: None)
    frames = [torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((6, 10, 3), dtype=torch.uint8)]
    boxes = torch.zeros((2, 3, 4))
    scores, count = torch.zeros((2, 3)), torch.zeros((2,), dtype=torch.int32)
    labels, numbers = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int32)
    draw = cl.draw_detections
    bad_calls = {
        "boxes dtype": lambda: draw(frames, boxes.double()),
        "boxes shape": lambda: draw(frames, torch.zeros((2, 3, 5))),
        "boxes 2-d": lambda: draw(frames, torch.zeros((2, 4))),
        "boxes not contiguous": lambda: draw(frames, torch.zeros((2, 3, 8))[..., ::2]),
        "boxes not a tensor": lambda: draw(frames, boxes.numpy()),
        "N mismatch": lambda: draw(frames, torch.zeros((3, 3, 4))),
        "boxes on another device": lambda: draw(frames, torch.zeros((2, 3, 4), device="meta")),
        "frames on different devices": lambda: draw([frames[0], torch.zeros((8, 8, 3), dtype=torch.uint8, device="meta")], boxes),
        "frames dtype": lambda: draw([f.float() for f in frames], boxes),
        "frames mixed C": lambda: draw([frames[0], torch.zeros((8, 8, 4), dtype=torch.uint8)], boxes),
        "frames C = 2": lambda: draw([torch.zeros((8, 8, 2), dtype=torch.uint8)] * 2, boxes),
        "frames C = 1": lambda: draw([torch.zeros((8, 8, 1), dtype=torch.uint8)] * 2, boxes),
        "frames C = 5": lambda: draw([torch.zeros((8, 8, 5), dtype=torch.uint8)] * 2, boxes),
        "tensor C = 2": lambda: draw(torch.zeros((2, 8, 8, 2), dtype=torch.uint8), boxes),
        "tensor not 4-d": lambda: draw(torch.zeros((8, 8, 3), dtype=torch.uint8), boxes),
        "tensor dtype": lambda: draw(torch.zeros((2, 8, 8, 3)), boxes),
        "empty frame": lambda: draw([torch.zeros((0, 8, 3), dtype=torch.uint8)] * 2, boxes),
        "frame side > 32768": lambda: draw([torch.zeros((1, 32769, 3), dtype=torch.uint8)] * 2, boxes),
        "in place, pixels not packed": lambda: draw([torch.zeros((8, 8, 6), dtype=torch.uint8)[..., ::2]] * 2, boxes, inplace=True),
        "in place, columns strided": lambda: draw([torch.zeros((8, 16, 3), dtype=torch.uint8)[:, ::2]] * 2, boxes, inplace=True),
        "scores without threshold": lambda: draw(frames, boxes, scores=scores),
        "threshold without scores": lambda: draw(frames, boxes, score_threshold=0.3),
        "threshold NaN": lambda: draw(frames, boxes, scores=scores, score_threshold=float("nan")),
        "scores shape": lambda: draw(frames, boxes, scores=torch.zeros((2, 4)), score_threshold=0.3),
        "scores dtype": lambda: draw(frames, boxes, scores=scores.double(), score_threshold=0.3),
        "scores device": lambda: draw(frames, boxes, scores=torch.zeros((2, 3), device="meta"), score_threshold=0.3),
        "count dtype": lambda: draw(frames, boxes, count=count.long()),
        "count shape": lambda: draw(frames, boxes, count=torch.zeros((3,), dtype=torch.int32)),
        "labels dtype": lambda: draw(frames, boxes, labels=labels.int()),
        "labels shape": lambda: draw(frames, boxes, labels=torch.zeros((2, 4), dtype=torch.int64)),
        "labels device": lambda: draw(frames, boxes, labels=torch.zeros((2, 3), dtype=torch.int64, device="meta")),
        "numbers dtype": lambda: draw(frames, boxes, numbers=numbers.long()),
        "numbers shape": lambda: draw(frames, boxes, numbers=torch.zeros((3, 3), dtype=torch.int32)),
        "numbers not a tensor": lambda: draw(frames, boxes, numbers=[[1, 2, 3], [4, 5, 6]]),
        "thickness 0": lambda: draw(frames, boxes, thickness=0),
        "thickness 33": lambda: draw(frames, boxes, thickness=33),
        "thickness float": lambda: draw(frames, boxes, thickness=2.0),
        "fill_alpha -1": lambda: draw(frames, boxes, fill_alpha=-1),
        "fill_alpha 257": lambda: draw(frames, boxes, fill_alpha=257),
        "tag_scale -1": lambda: draw(frames, boxes, tag_scale=-1),
        "tag_scale 9": lambda: draw(frames, boxes, tag_scale=9),
        "palette empty": lambda: draw(frames, boxes, palette=[]),
        "palette 257 entries": lambda: draw(frames, boxes, palette=[(1, 2, 3)] * 257),
        "palette [P, 4]": lambda: draw(frames, boxes, palette=[(1, 2, 3, 4)]),
        "palette value 256": lambda: draw(frames, boxes, palette=[(1, 2, 256)]),
        "palette floats": lambda: draw(frames, boxes, palette=[(0.5, 0.5, 0.5)]),
        "text colour": lambda: draw(frames, boxes, text_color=(255, 255)),
        "pixel format": lambda: draw(frames, boxes, pixel_format="yv12"),
        "matrix": lambda: draw([yuv_planes(4, 8)] * 2, boxes, pixel_format="nv12", matrix="bt2020"),
        "packed RGB with a YUV format": lambda: draw(frames, boxes, pixel_format="i420"),
        "odd YUV frame": lambda: draw([torch.zeros((9, 7), dtype=torch.uint8)] * 2, boxes, pixel_format="nv12"),
        "YUV N mismatch": lambda: draw([yuv_planes(4, 8)], boxes, pixel_format="i420"),
        "pitched I420 tensor in place": lambda: draw([torch.zeros((6, 16), dtype=torch.uint8)[:, :8]] * 2, boxes, pixel_format="i420", inplace=True),
    }
    for what, bad in bad_calls.items():
        with pytest.raises(ValueError):
            bad()
            pytest.fail(f"{what}: not refused")


def test_an_empty_batch_is_returned_without_a_device():
    assert cl.draw_detections([], torch.zeros((0, 5, 4))) == []
    assert cl.draw_detections([], torch.zeros((0, 5, 4)), pixel_format="nv12", inplace=True) == []
    with pytest.raises(ValueError):
        cl.draw_detections([], torch.zeros((1, 5, 4)))
