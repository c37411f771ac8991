"""Host: the "write only your slice" harness (tests/strided_io.py) catches what it is for.  A torch CPU stand-in plays the kernel: a correct one
passes; one that also writes ONE element into a padding channel, into the pixel after the last, or into the guard before is flagged at that place.
The same for the byte-granular guard (GuardedBytes) and for the strided [N, C, H, W] views (StridedView)."""
import ctypes

import pytest
import torch

from strided_io import GUARD_PIXELS, POISONS, SENTINEL, VIEW_LAYOUTS, Guarded, GuardedBytes, StridedView, record_mask

N, H, W, C = 2, 3, 5, 20


def _x():
    return torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(1))


def _stand_in(x, y, stray=None):
    """y = 2 x + 1 through the strided views, as a kernel addresses them: base pointer + pixel * ld + channel."""
    y.view.copy_(2 * x.view + 1)
    if stray is not None:
        flat = y.alloc
        base = y.guard + y.off                          # the slice pointer
        flat[base + stray] = 7.0


@pytest.mark.parametrize("ld,off", [(C, 0), (C + 4, 4), (C + 12, 4), (C + 3, 3), (C + 12, 0)])
def test_a_correct_stand_in_passes(ld, off):
    x = Guarded((N, H, W), C, ld + 4, off, data=_x(), name="x")
    y = Guarded((N, H, W), C, ld, off)
    assert y.untouched() and y.unwritten() == N * H * W * C
    assert y.aligned16 == (off % 4 == 0) and y.alloc.numel() == (2 * GUARD_PIXELS + N * H * W) * ld
    _stand_in(x, y)
    ok, msg = y.verdict()
    assert ok, msg
    assert x.unchanged() and y.unwritten() == 0 and not y.untouched()
    assert torch.equal(y.result(), 2 * _x() + 1)
    assert not torch.isnan(y.result()).any()
    # the input: NaN everywhere outside its slice
    outside = torch.ones(x.alloc.numel(), dtype=torch.bool)
    outside.as_strided(x.view.shape, x.view.stride(), x.guard + x.off).fill_(False)
    assert bool(torch.isnan(x.alloc[outside]).all()) and not torch.isnan(x.view).any()
    y.refill()
    assert y.untouched()


def test_one_element_in_a_padding_channel_is_flagged_there():
    ld, off = C + 12, 4
    y = Guarded((N, H, W), C, ld, off)
    pix = (1 * H + 2) * W + 3                                   # image 1, row 2, column 3
    _stand_in(Guarded((N, H, W), C, data=_x()), y, stray=pix * ld + C + 1)          # the second channel past the slice
    ok, msg = y.verdict()
    assert not ok and "1 word(s)" in msg and f"first at (1, 2, 3, {C + 1})" in msg and f"last at (1, 2, 3, {C + 1})" in msg, msg
    # ... and in the channels before the slice of a pixel: the kernel sees them as the tail of the pixel before
    y = Guarded((N, H, W), C, ld, off)
    _stand_in(Guarded((N, H, W), C, data=_x()), y, stray=pix * ld - 1)
    ok, msg = y.verdict()
    assert not ok and f"first at (1, 2, 2, {ld - 1})" in msg, msg


def test_one_element_in_the_pixel_after_the_last_is_flagged_as_guard_after():
    for ld, off in ((C, 0), (C + 3, 3)):
        y = Guarded((N, H, W), C, ld, off)
        _stand_in(Guarded((N, H, W), C, data=_x()), y, stray=N * H * W * ld + 2)       # channel 2 of pixel N H W
        ok, msg = y.verdict()
        assert not ok and "first at guard after" in msg and "last at guard after" in msg, msg
    # the padding channels of the LAST pixel are still the tensor's own body
    y = Guarded((N, H, W), C, C + 4, 0)
    _stand_in(Guarded((N, H, W), C, data=_x()), y, stray=(N * H * W - 1) * (C + 4) + C)
    ok, msg = y.verdict()
    assert not ok and f"first at ({N - 1}, {H - 1}, {W - 1}, {C})" in msg, msg


def test_one_element_in_the_guard_before_is_flagged():
    for ld, off, stray in ((C, 0, -1), (C + 4, 4, -5), (C + 4, 4, -GUARD_PIXELS * (C + 4) - 4)):
        y = Guarded((N, H, W), C, ld, off)
        _stand_in(Guarded((N, H, W), C, data=_x()), y, stray=stray)
        ok, msg = y.verdict()
        assert not ok and "first at guard before" in msg and "last at guard before" in msg, msg


def test_first_and_last_offender_are_both_reported():
    y = Guarded((N, H, W), C, C + 4, 0)
    _stand_in(Guarded((N, H, W), C, data=_x()), y)
    y.alloc[y.guard - 3] = 1.0
    y.alloc[y.guard + 0 * (C + 4) + C] = 1.0
    y.alloc[y.guard + y.body + 9] = 1.0
    ok, msg = y.verdict()
    assert not ok and "3 word(s)" in msg and "first at guard before" in msg and "last at guard after" in msg, msg


def test_only_mask_for_slot_arrays():
    """The y_absmax arrays: a line of 32 floats per image, only element 0 of each may change."""
    ams = 32
    slots = Guarded((N,), ams, name="y_absmax")
    only = torch.zeros(ams, dtype=torch.bool)
    only[0] = True
    slots.view[:, 0] = torch.tensor([3.0, 4.0])
    ok, msg = slots.verdict(only)
    assert ok, msg
    slots.view[1, 5] = 0.0
    ok, msg = slots.verdict(only)
    assert not ok and "first at (1, 5)" in msg, msg


def test_a_written_sentinel_free_result_and_a_nan_are_told_apart():
    """A NaN a kernel computes (0 * inf, a poisoned padding channel read) is the canonical NaN, never the sentinel: it counts as written."""
    y = Guarded((1, 1, 2), 4)
    y.view.copy_(torch.tensor([float("inf")]) * 0)
    assert y.unwritten() == 0 and bool(torch.isnan(y.result()).all())
    assert int(torch.tensor([float("nan")]).view(torch.int32)) != SENTINEL


# ------------------------------------------------------------------------------------------------------------------------ byte-level guards
@pytest.mark.parametrize("align", [4, 8, 16, 256])
@pytest.mark.parametrize("nbytes", [0, 1, 52, 4096])
def test_the_byte_guard_sits_at_exactly_its_alignment(align, nbytes):
    g = GuardedBytes(nbytes, align=align)
    assert g.ptr % align == 0 and g.ptr % (2 * align) != 0
    assert g.start >= 4096 and g.alloc.numel() - g.start - nbytes >= 4096
    assert g.untouched() and g.unwritten() == nbytes and g.body.numel() == nbytes
    ok, msg = g.verdict()
    assert ok, msg


def test_a_clean_write_of_mixed_records_passes():
    """Records of 52 bytes 64 apart (an int32 count, four float64, three float32): only the records may change, the gaps stay sentinel."""
    n, rec, stride = 3, 52, 64
    g = GuardedBytes(n * stride, align=8, mask=record_mask(n, stride, rec))
    for r in range(n):
        b = g.body[r * stride:r * stride + rec]
        b[:4].view(torch.int32).fill_(r + 1)
        b[8:40].view(torch.float64).copy_(torch.arange(4, dtype=torch.float64))
        b[40:52].view(torch.float32).fill_(1.5)
    ok, msg = g.verdict()
    assert ok, msg
    assert g.unwritten() == n * 4                                   # bytes 4..8 of each record: never stored
    assert not g.untouched()
    assert g.result(torch.int32, (1,)).item() == 1
    g.refill()
    assert g.untouched()


@pytest.mark.parametrize("where,offset,text", [("before", -1, "guard before (byte -1)"), ("before_far", -4096, "guard before (byte -4096)"),
                                               ("after", 0, "guard after (byte 0 past the end)"), ("after_far", 4095, "guard after (byte 4095 past the end)"),
                                               ("gap", 52, "body byte 52"), ("gap_last", 3 * 64 - 1, "body byte 191"), ("masked_off", 64 + 40, "body byte 104")])
def test_one_stray_byte_is_caught_and_located(where, offset, text):
    n, rec, stride = 3, 52, 64
    used = [52, 40, 52] if where == "masked_off" else 52            # record 1 is written only up to byte 40: a store behind that is stray
    g = GuardedBytes(n * stride, align=16, mask=record_mask(n, stride, used))
    for r in range(n):
        g.body[r * stride:r * stride + 40] = 7
    pos = g.start + (g.nbytes + offset if where.startswith("after") else offset)
    g.alloc[pos] = 0
    ok, msg = g.verdict()
    assert not ok and "1 byte(s)" in msg and f"first at {text}" in msg and f"last at {text}" in msg, msg


def test_first_and_last_stray_byte_are_both_reported_and_the_sentinel_is_selectable():
    for sentinel in (0xA5, 0x3C):
        g = GuardedBytes(100, align=4, sentinel=sentinel, mask=record_mask(1, 100, 60))
        assert int(g.alloc[0]) == sentinel
        g.body[:60] = 1
        g.alloc[g.start - 7] = 0
        g.body[99] = 0
        ok, msg = g.verdict()
        assert not ok and "2 byte(s)" in msg and "first at guard before (byte -7)" in msg and "last at body byte 99" in msg, msg
        ok, _ = g.verdict(mask=record_mask(1, 100, 100))           # a wider mask at the call: byte 99 is allowed, the guard byte still is not
        assert not ok
    g = GuardedBytes(8, align=8)
    g.typed(torch.float64).fill_(0.0)
    g.body[3] = 0xA5                                                # a result that happens to contain the sentinel byte: not an error, one "unwritten"
    assert g.verdict()[0] and g.unwritten() == 1


def test_the_byte_guard_wraps_memory_it_does_not_own():
    """The mapped host memory of cnl_host_alloc: the guard lives inside a caller's pointer (here: a ctypes buffer)."""
    need = GuardedBytes.wrapped_bytes(200, align=8)
    buf = (ctypes.c_uint8 * (need + 64))()
    g = GuardedBytes(200, align=8, wrap=(ctypes.addressof(buf), need + 64), name="record")
    assert g.ptr % 8 == 0 and g.ptr % 16 != 0 and ctypes.addressof(buf) + 4096 <= g.ptr
    assert g.untouched() and buf[0] == 0xA5
    ctypes.memset(g.ptr, 1, 200)                                    # the "kernel" writes through the raw pointer
    assert g.verdict()[0] and g.unwritten() == 0
    ctypes.memset(g.ptr + 200, 1, 1)
    ok, msg = g.verdict()
    assert not ok and "record" in msg and "guard after (byte 0 past the end)" in msg, msg
    with pytest.raises(AssertionError):
        GuardedBytes(200, align=8, wrap=(ctypes.addressof(buf), 200))


# ------------------------------------------------------------------------------------------------------------------------ strided views
def _addressed(v, N, C, H, W):
    """Gather every element through (pointer, strides) alone, as a kernel does."""
    base = (v.ptr - v.alloc.data_ptr()) // 4
    sn, sc, sh, sw = v.strides
    n, c, y, x = torch.meshgrid(torch.arange(N), torch.arange(C), torch.arange(H), torch.arange(W), indexing="ij")
    return base + n * sn + c * sc + y * sh + x * sw


@pytest.mark.parametrize("poison", ["inf", "nan", "big"])
@pytest.mark.parametrize("layout", VIEW_LAYOUTS)
def test_a_view_addresses_exactly_its_data_with_poison_everywhere_else(layout, poison):
    N, C, H, W = 2, 5, 3, 4
    data = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(3))
    v = StridedView(data, layout, poison)
    idx = _addressed(v, N, C, H, W)
    assert int(idx.min()) >= 4096 and int(idx.max()) < v.alloc.numel() - 4096
    assert idx.unique().numel() == N * C * H * W                   # no two elements share a word
    assert torch.equal(v.alloc[idx], data) and torch.equal(v.view, data)
    outside = torch.ones(v.alloc.numel(), dtype=torch.bool)
    outside[idx.reshape(-1)] = False
    rest = v.alloc[outside]
    want = torch.full((1,), POISONS[poison])
    assert bool((rest.view(torch.int32) == want.view(torch.int32)).all())
    assert v.unchanged()
    v.alloc[0] = 1.0
    assert not v.unchanged()


def test_the_layouts_differ_from_packed_the_way_the_table_says():
    N, C, H, W = 2, 8, 6, 8
    data = torch.zeros(N, C, H, W)
    s = {name: StridedView(data, name) for name in VIEW_LAYOUTS}
    a = {name: (v.ptr - v.alloc.data_ptr()) % 16 for name, v in s.items()}
    assert s["nchw"].strides == (C * H * W, H * W, W, 1) and s["nhwc"].strides == (H * W * C, 1, W * C, C) and s["nchw"].packed and s["nhwc"].packed
    assert s["nhwc_wide"].strides == (H * W * (C + 12), 1, W * (C + 12), C + 12) and a["nhwc_wide"] == 0
    assert s["nhwc_off1"].strides[3] == C + 7 and a["nhwc_off1"] == 4
    assert s["nhwc_off2"].strides[3] == C + 6 and a["nhwc_off2"] == 8
    assert s["nhwc_ld3"].strides[3] == C + 3 and a["nhwc_ld3"] == 12
    v = StridedView(data, "nhwc+4+6")
    assert v.strides == (H * W * (C + 6), 1, W * (C + 6), C + 6) and (v.ptr - v.alloc.data_ptr()) % 16 == 0 and not v.packed
    assert s["nchw_window"].strides == (C * (H + 3) * (W + 8), (H + 3) * (W + 8), W + 8, 1) and a["nchw_window"] == 0
    assert s["nchw_window_odd"].strides == (C * (H + 3) * (W + 5), (H + 3) * (W + 5), W + 5, 1) and a["nchw_window_odd"] == ((W + 5 + 1) * 4) % 16
    assert s["batch_slice"].strides == s["nhwc"].strides and s["batch_slice_nchw"].strides == s["nchw"].strides
    assert s["batch_every_other"].strides[0] == 2 * H * W * C and s["batch_every_other_nchw"].strides[0] == 2 * C * H * W
    assert s["every_other_pixel_nchw"].strides == (4 * C * H * W, 4 * H * W, 4 * W, 2)
    assert s["every_other_pixel_nhwc"].strides == (4 * H * W * C, 1, 4 * W * C, 2 * C)
    assert s["every_other_channel"].strides == (H * W * 2 * C, 2, W * 2 * C, 2 * C) and a["every_other_channel"] == 0
    assert not any(v.packed for name, v in s.items() if name not in ("nchw", "nhwc"))
