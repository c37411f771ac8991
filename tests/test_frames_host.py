"""No GPU: the frame source (_frames.open_frames) and the record packer (_gather.pack_records) that letterbox, tile, crop and draw share.
The records are decoded with the ctypes structs of the C ABI and compared with addresses, pitches and sizes worked out here from
data_ptr(), stride() and the shapes; the device check is switched off, as in the other host tests, so host tensors stand in."""
import os

import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl
from centernet_lightning_amd import _frames, _gather, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (6, 10), (16, 8)]
FORMS = ["nv12", "i420", "nv12_surface", "y_uv", "y_u_v"]


@pytest.fixture(autouse=True)
def no_device_check(monkeypatch):
    monkeypatch.setattr(_gather, "require_hip", lambda tensors, what: None)


def pitched(shape, extra):
    """A view with the given shape inside a buffer whose rows are `extra` elements of dimension 1 longer."""
    return torch.zeros((shape[0], shape[1] + extra) + tuple(shape[2:]), dtype=torch.uint8)[:, :shape[1]]


def packed_frames(C=3):
    """Contiguous frames of SIZES, the middle one a row-pitched view."""
    return [torch.zeros((2, 2, C), dtype=torch.uint8), pitched((6, 10, C), 7), torch.zeros((16, 8, C), dtype=torch.uint8)]


def yuv_frames(form):
    out = []
    for i, (h, w) in enumerate(SIZES):
        if form in ("nv12", "i420"):
            out.append(torch.zeros((h * 3 // 2, w), dtype=torch.uint8))
        elif form == "nv12_surface":
            out.append(pitched((h * 3 // 2, w), 64 + 2 * i))
        elif form == "y_uv":
            out.append((pitched((h, w), 37 + i), pitched((h // 2, w // 2, 2), 5 + i)))
        else:
            out.append((pitched((h, w), 13 + i), pitched((h // 2, w // 2), 9), pitched((h // 2, w // 2), 9)))
    return out


def layout_of(form):
    return "i420" if form in ("i420", "y_u_v") else "nv12"


def pitch_of(rows, stride, row_bytes):
    """The record's rule: the row stride, or the packed width of a plane that has one row."""
    return stride if rows > 1 else row_bytes


def expected_planes(frame, form, h, w):
    """(y, u, v, y_pitch, c_pitch, c_step) of one frame of yuv_frames(form), from its tensors alone."""
    step = 2 if layout_of(form) == "nv12" and w > 2 else 1           # (a one-column chroma plane has no element stride)
    if form in ("nv12", "nv12_surface"):
        base, s = frame.data_ptr(), frame.stride(0)
        return (base, base + h * s, base + h * s + 1, s, pitch_of(h // 2, s, w // 2 * step), step)
    if form == "i420":
        base = frame.data_ptr()
        return (base, base + h * w, base + h * w + (h // 2) * (w // 2), w, w // 2, 1)
    if form == "y_uv":
        y, uv = frame
        return (y.data_ptr(), uv.data_ptr(), uv.data_ptr() + 1, y.stride(0), pitch_of(h // 2, uv.stride(0), w // 2 * step), step)
    y, u, v = frame
    return (y.data_ptr(), u.data_ptr(), v.data_ptr(), y.stride(0), pitch_of(h // 2, u.stride(0), w // 2), 1)


def odd_window(n, h, w):
    return (n, 1, 1, h - 1, w - 1, 3, 5, 7, 9)


def window_sets(src):
    return [src.whole(), [odd_window(1, *SIZES[1])], [odd_window(n, h, w) for n, (h, w) in enumerate(SIZES)]]


# ----------------------------------------------------------------------------- the packer against the structs
@pytest.mark.parametrize("C", [1, 3, 4])
def test_packed_records_decode_to_the_frames_addresses_and_pitches(C):
    frames = packed_frames(C)
    src = _frames.open_frames(frames, "rgb", "test", copy=_frames.ROWS)
    assert (src.kind, src.C, src.sizes, src.coef, len(src)) == (_frames.PACKED, C, SIZES, None, 3)
    assert src.whole() == [(n, 0, 0, h, w, 1, 1, 0, 0) for n, (h, w) in enumerate(SIZES)]
    assert frames[1].stride(0) == (10 + 7) * C                       # the pitched frame really is pitched
    for windows in window_sets(src):
        plain, planes = src.records(windows)
        assert planes is None
        buf = _gather.pack_records(windows, plain, planes, tail_words=3)
        assert buf.dtype == np.int64 and buf.shape == (len(windows) * 5 + 3,) and (buf[len(windows) * 5:] == 0).all()
        got = (_lib.LetterboxFrame * len(windows)).from_buffer_copy(buf[:len(windows) * 5].tobytes())
        for g, (n, y0, x0, h, w, nh, nw, pt, pl) in zip(got, windows):
            f = frames[n]
            stride = pitch_of(f.shape[0], f.stride(0), f.shape[1] * C)
            assert g.src == f.data_ptr() + y0 * stride + x0 * C
            assert (g.h, g.w, g.row_stride, g.new_h, g.new_w, g.pad_top, g.pad_left, g.reserved) == (h, w, stride, nh, nw, pt, pl, 0)


@pytest.mark.parametrize("form", FORMS)
def test_yuv_records_decode_to_the_planes_addresses_and_pitches(form):
    frames = yuv_frames(form)
    src = _frames.open_frames(frames, layout_of(form), "test", "bt709", True)
    assert (src.kind, src.C, src.sizes, len(src)) == (_frames.YUV, 3, SIZES, 3)
    assert src.coef == cl.yuv_coefficients("bt709", True)
    want = [expected_planes(f, form, h, w) for f, (h, w) in zip(frames, SIZES)]
    for windows in window_sets(src):
        V = len(windows)
        plain, planes = src.records(windows)
        buf = _gather.pack_records(windows, plain, planes)
        assert buf.dtype == np.int64 and buf.shape == (V * 9,)
        for g, (n, y0, x0, h, w, nh, nw, pt, pl) in zip((_lib.Yuv420Frame * V).from_buffer_copy(buf.tobytes()), windows):
            assert (g.y, g.u, g.v, g.y_pitch, g.c_pitch, g.c_step) == want[n], (form, n)
            assert (g.x0, g.y0, g.h, g.w, g.new_h, g.new_w, g.pad_top, g.pad_left, g.reserved) == (x0, y0, h, w, nh, nw, pt, pl, 0)
        # the same windows as packed one-channel frames: the Y plane (what unletterbox's table holds)
        buf = _gather.pack_records(windows, plain)
        for g, (n, y0, x0, h, w, nh, nw, pt, pl) in zip((_lib.LetterboxFrame * V).from_buffer_copy(buf.tobytes()), windows):
            assert g.src == want[n][0] + y0 * want[n][3] + x0 and g.row_stride == want[n][3]
            assert (g.h, g.w, g.new_h, g.new_w, g.pad_top, g.pad_left) == (h, w, nh, nw, pt, pl)


def test_a_pitched_i420_tensor_is_split_planes_one_copy():
    surface = pitched((9, 10), 6)                                     # h = 6, w = 10: the chroma planes are flat byte ranges
    src = _frames.open_frames([surface], "i420", "test")
    (y, u, v), = src.keep
    assert y.data_ptr() != surface.data_ptr() and (y.stride(0), u.stride(0)) == (10, 5)
    assert src.records(src.whole()) == ([(y.data_ptr(), 10)], [(y.data_ptr(), y.data_ptr() + 60, y.data_ptr() + 75, 10, 5, 1)])


# ----------------------------------------------------------------------------- the copy rules
def test_copy_rules():
    C = 3
    rows = pitched((6, 10, C), 7)                                     # rows strided, pixels packed
    cols = torch.zeros((6, 20, C), dtype=torch.uint8)[:, ::2]         # columns strided
    for rule in (_frames.ROWS, _frames.IN_PLACE):                    # tile_uint8's rule and draw_detections(inplace=True)'s
        src = _frames.open_frames([rows], "rgb", "test", copy=rule)
        assert src.keep[0].data_ptr() == rows.data_ptr() and src.keep[0].stride() == rows.stride()
        assert src.records(src.whole()) == ([(rows.data_ptr(), 17 * C)], None)
    src = _frames.open_frames([rows], "rgb", "test")                  # letterbox_uint8's and crop_detections' rule
    assert src.keep[0].data_ptr() != rows.data_ptr() and src.keep[0].is_contiguous()
    assert src.records(src.whole()) == ([(src.keep[0].data_ptr(), 10 * C)], None)
    src = _frames.open_frames([cols], "rgb", "test", copy=_frames.ROWS)
    assert src.keep[0].data_ptr() != cols.data_ptr() and src.keep[0].is_contiguous() and src.records(src.whole())[0][0][1] == 10 * C
    with pytest.raises(ValueError, match="in place"):
        _frames.open_frames([cols], "rgb", "test", copy=_frames.IN_PLACE)
    # one column has no pixel stride: the in-place draw rule takes any, the tile rule copies the frame unless it is C (as it always did)
    one = torch.zeros((6, 2, C), dtype=torch.uint8)[:, ::2]
    assert tuple(one.shape) == (6, 1, C) and one.stride() == (2 * C, 2 * C, 1)
    src = _frames.open_frames([one], "rgb", "test", copy=_frames.IN_PLACE)
    assert src.records(src.whole()) == ([(one.data_ptr(), 2 * C)], None)
    src = _frames.open_frames([one], "rgb", "test", copy=_frames.ROWS)
    assert src.keep[0].data_ptr() != one.data_ptr() and src.records(src.whole()) == ([(src.keep[0].data_ptr(), C)], None)
    # a batch tensor: made contiguous as a whole under the dense rule, read where it lies under the other two
    batch = torch.zeros((2, 6, 17, C), dtype=torch.uint8)[:, :, :10]
    for rule in (_frames.ROWS, _frames.IN_PLACE):
        src = _frames.open_frames(batch, "rgb", "test", copy=rule)
        assert [f.data_ptr() for f in src.keep] == [batch[0].data_ptr(), batch[1].data_ptr()]
    src = _frames.open_frames(batch, "rgb", "test")
    assert src.keep[1].data_ptr() - src.keep[0].data_ptr() == 6 * 10 * C
    # a pitched form-(a) I420 tensor is refused in place (split_planes copies it); its planes are not
    with pytest.raises(ValueError, match="contiguous"):
        _frames.open_frames([pitched((9, 10), 6)], "i420", "test", copy=_frames.IN_PLACE)
    y, u, v = pitched((6, 10), 3), pitched((3, 5), 2), pitched((3, 5), 2)
    assert _frames.open_frames([(y, u, v)], "i420", "test", copy=_frames.IN_PLACE).keep[0][0].data_ptr() == y.data_ptr()
    # empty batches
    for fmt in ("rgb", "nv12"):
        with pytest.raises(ValueError, match="no frames"):
            _frames.open_frames([], fmt, "test")
        src = _frames.open_frames([], fmt, "test", allow_empty=True)
        assert len(src) == 0 and src.device is None and src.whole() == []


# ----------------------------------------------------------------------------- one source behind the four gathers
def test_the_four_gathers_hand_over_the_sources_records(monkeypatch):
    seen = {}

    class Captured(Exception):
        pass

    def fake_gather(dev, windows, plain, height, width, C, word, planes=None, coef=None, merge_records=None, frame_first_view=None):
        seen.update(windows=windows, plain=plain, planes=planes, coef=coef, C=C)
        raise Captured

    monkeypatch.setattr(_gather, "gather", fake_gather)
    sizes = [(40, 70), (2, 2), (33, 100)]
    dense = [torch.zeros((h, w, 3), dtype=torch.uint8) for (h, w) in sizes]
    strided = [dense[0], pitched((2, 2, 3), 5), pitched((33, 100, 3), 1)]
    yuv = [(pitched((40, 70), 3), pitched((20, 35, 2), 1)), torch.zeros((3, 2), dtype=torch.uint8), pitched((48, 100), 28)]
    cases = [(lambda: cl.letterbox.letterbox_uint8(dense, 32, 64), _frames.open_frames(dense, "rgb", "test")),
             (lambda: cl.tile_uint8(strided, 32, 32, 0.1), _frames.open_frames(strided, "rgb", "test", copy=_frames.ROWS)),
             (lambda: cl.letterbox_yuv420(yuv, 32, 64, matrix="bt709"), _frames.open_frames(yuv, "nv12", "test", "bt709")),
             (lambda: cl.tile_yuv420(yuv, 32, 32, 0.1, matrix="bt709"), _frames.open_frames(yuv, "nv12", "test", "bt709"))]
    for call, src in cases:
        seen.clear()
        with pytest.raises(Captured):
            call()
        assert len(seen["windows"]) >= len(sizes) and (seen["plain"], seen["planes"]) == src.records(seen["windows"])
        assert (seen["coef"], seen["C"]) == (src.coef, 3) and (seen["planes"] is None) == (src.kind == _frames.PACKED)
    assert any(y0 % 2 or x0 % 2 for (_, y0, x0, *_) in seen["windows"])            # the tiles include odd origins


# ----------------------------------------------------------------------------- one dispatch
def test_an_unknown_pixel_format_is_refused_alike_everywhere():
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    frames, boxes = [torch.zeros((8, 8, 3), dtype=torch.uint8)], torch.zeros((1, 2, 4))
    for call in (lambda: cl.crop_detections(frames, boxes, pixel_format="yv12"), lambda: cl.draw_detections(frames, boxes, pixel_format="yv12"),
                 lambda: model.detect_frames(frames, 32, 32, pixel_format="yv12"), lambda: model.detect_tiled(frames, tile=(32, 32), pixel_format="yv12")):
        with pytest.raises(ValueError, match="pixel_format must be 'rgb' or one of"):
            call()
    for name in ("letterbox.py", "tiles.py", "yuv.py", "crops.py", "overlay.py", "models.py", "_gather.py", "_frames.py"):
        text = open(os.path.join(ROOT, "centernet-lightning_amd", "centernet_lightning_amd", name)).read()
        assert text.count("pixel_format must be") == (1 if name == "_frames.py" else 0), name
