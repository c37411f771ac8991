"""Host: the "write only your slice" harness (tests/strided_io.py) catches what it is for.  A torch CPU stand-in plays the kernel: a correct one
passes; one that also writes ONE element into a padding channel, into the pixel after the last, or into the guard before is flagged at that place."""
import pytest
import torch

from strided_io import GUARD_PIXELS, SENTINEL, Guarded

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
