"""A "write only your slice" harness for the kernels of the C ABI (plain helper: no fixtures).

Every tensor of a launch is a channel slice [off, off + C) of a wider row-major buffer with pixel stride ld >= off + C, and the buffer sits inside ONE
larger allocation with a guard band of GUARD_PIXELS x ld floats before and after it (the slack the launchers themselves reserve in their span checks,
and enough for a stray tile row to stay inside memory the test owns):

    [ guard before | pixel 0: off pad, C slice, ld - off - C pad | pixel 1 ... | pixel P-1 ... | guard after ]

An INPUT carries its data in the slice and NaN everywhere else.  An OUTPUT is filled, slice included, with one sentinel bit pattern that no result can
equal (a NaN with a chosen payload: arithmetic produces the canonical quiet NaN or propagates its operands' payloads, and no operand carries this one);
after the launch Guarded.verdict() compares the allocation as int32 words: every word outside the slice must still hold the sentinel.  Offsets are
reported the way the kernel sees the tensor, relative to the slice pointer: (leading indices..., channel) with channel >= C a padding channel, or
"guard before" / "guard after".  `only` restricts the words that may change further (the y_absmax arrays: element 0 of each 32-float line).

The same code runs on the CPU (tests/test_strided_io_host.py plants stray writes with torch) and on the GPU."""
import math

import torch

SENTINEL = 0x7FC5A5A5          # a quiet NaN with the payload 0x45A5A5 (positive as int32)
GUARD_PIXELS = 512


def _sentinel_fill(t):
    t.view(torch.int32).fill_(SENTINEL)
    return t


class Guarded:
    """A [*lead, C] tensor (row-major over the leading dims, pixel stride ld floats) at channel offset `off` of a wider buffer, with guards.

    data: None -> an output (sentinel everywhere); a CPU / device tensor of shape [*lead, C] -> an input (NaN outside the slice)."""

    def __init__(self, lead, C, ld=None, off=0, data=None, device="cpu", guard_pixels=GUARD_PIXELS, name="y"):
        self.lead = tuple(int(v) for v in lead)
        self.C, self.off, self.name = int(C), int(off), name
        self.ld = int(ld) if ld is not None else self.C + self.off
        assert self.ld >= self.off + self.C and self.C > 0
        self.P = math.prod(self.lead)
        self.guard = guard_pixels * self.ld
        assert self.guard % 4 == 0          # (the allocation is 16-byte aligned: the slice pointer is 16-byte aligned exactly when off % 4 == 0)
        self.body = self.P * self.ld
        self.alloc = torch.empty(2 * self.guard + self.body, dtype=torch.float32, device=device)
        if data is None:
            _sentinel_fill(self.alloc)
        else:
            self.alloc.fill_(float("nan"))
            self.view.copy_(data.to(device=device, dtype=torch.float32).reshape(*self.lead, self.C))
        self.snapshot = self.alloc.clone() if data is not None else None

    @property
    def view(self):
        """The slice: [*lead, C], strides of the wider buffer."""
        strides, s = [], self.ld
        for d in reversed(self.lead):
            strides.append(s)
            s *= d
        return self.alloc.as_strided(self.lead + (self.C,), tuple(reversed(strides)) + (1,), self.guard + self.off)

    @property
    def ptr(self):
        return self.alloc.data_ptr() + 4 * (self.guard + self.off)

    @property
    def aligned16(self):
        return self.ptr % 16 == 0

    def refill(self):
        """An output: back to all sentinel (between two launches into the same allocation)."""
        assert self.snapshot is None
        _sentinel_fill(self.alloc)

    def where(self, word):
        """Offset of one float of the allocation as the kernel addresses it (relative to the slice pointer)."""
        k = int(word) - self.guard - self.off
        if k < 0:
            return "guard before" + (f" (the {self.off} floats before the slice pointer)" if word >= self.guard else "")
        pix, c = divmod(k, self.ld)
        if pix >= self.P:
            return "guard after"
        idx = []
        for d in reversed(self.lead):
            pix, r = divmod(pix, d)
            idx.append(r)
        return tuple(reversed(idx)) + (c,)

    def _allowed(self, only=None):
        m = torch.zeros(self.alloc.numel(), dtype=torch.bool, device=self.alloc.device)
        v = m.as_strided(self.view.shape, self.view.stride(), self.guard + self.off)
        if only is None:
            v.fill_(True)
        else:
            v.copy_(only.to(m.device).expand(v.shape))
        return m

    def verdict(self, only=None):
        """-> (ok, message).  ok: every int32 word outside the slice (outside `only`, a bool mask broadcastable to the slice) still holds the sentinel."""
        assert self.snapshot is None, "verdict() is for outputs; inputs: unchanged()"
        bad = (self.alloc.view(torch.int32) != SENTINEL) & ~self._allowed(only)
        n = int(bad.sum())
        if n == 0:
            return True, f"{self.name}: nothing outside the slice was written"
        idx = torch.nonzero(bad).reshape(-1)
        first, last = int(idx[0]), int(idx[-1])
        return False, (f"{self.name}: {n} word(s) outside the slice were written; first at {self.where(first)}, last at {self.where(last)} "
                       f"(slice [*{self.lead}, {self.C}] at channel offset {self.off}, pixel stride {self.ld})")

    def untouched(self):
        """An output no launch may have written at all (a rejected launch): every word is the sentinel."""
        return bool((self.alloc.view(torch.int32) == SENTINEL).all())

    def unwritten(self):
        """Words INSIDE the slice that still hold the sentinel (a launch that should have written all of it)."""
        return int((self.view.contiguous().view(torch.int32) == SENTINEL).sum())

    def unchanged(self):
        """An input: its whole allocation holds the bits it was built with."""
        return bool((self.alloc.view(torch.int32) == self.snapshot.view(torch.int32)).all())

    def result(self):
        """The slice on the CPU, contiguous."""
        return self.view.detach().cpu().contiguous()
