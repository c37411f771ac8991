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

The same code runs on the CPU (tests/test_strided_io_host.py plants stray writes with torch) and on the GPU.

GuardedBytes (below) is the byte-granular sibling for outputs and workspaces of any element type, StridedView a logical [N, C, H, W] fp32 view of wider,
poisoned storage in the layouts ordinary torch slicing produces."""
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


# ------------------------------------------------------------------------------------------------------------------------ byte-level guards
SENTINEL_BYTE = 0xA5
GUARD_BYTES = 4096


def record_mask(n_records, stride, used, nbytes=None):
    """A bool mask over the bytes of `n_records` records `stride` bytes apart: True for the first `used` bytes of each (`used` an int or one int per record)."""
    nbytes = n_records * stride if nbytes is None else nbytes
    m = torch.zeros(nbytes, dtype=torch.bool)
    for r in range(n_records):
        u = used if isinstance(used, int) else int(used[r])
        assert 0 <= u <= stride
        m[r * stride:r * stride + u] = True
    return m


class GuardedBytes:
    """`nbytes` of output / workspace of ANY element type, inside ONE allocation with a guard band before and after, all of it one sentinel byte:

        [ guard before (>= guard bytes) | body: nbytes, its first byte at an address that is a multiple of `align` and NOT of 2 * align | guard after ]

    so a pointer sits at exactly its documented alignment and no more.  `mask` (bool, one per body byte) names the body bytes that may change (records
    where only an n x T part is written, record strides larger than the record); None: the whole body.  verdict() compares bytes and reports the first
    and the last stray one as the kernel addresses them: "guard before", "guard after", or the byte offset in the body.  unwritten() counts the allowed
    body bytes that still hold the sentinel — a result may legitimately contain that byte, so callers compare with the oracle (or run two sentinels).

    wrap=(address, length): the allocation is `length` bytes of host-visible memory the caller owns at `address` (mapped host memory of
    cnl_host_alloc) instead of a torch allocation; the checks then read it from the CPU."""

    def __init__(self, nbytes, align=256, device="cpu", guard=GUARD_BYTES, sentinel=SENTINEL_BYTE, mask=None, name="out", wrap=None):
        assert nbytes >= 0 and align >= 1 and (align & (align - 1)) == 0 and 0 <= sentinel < 256
        self.nbytes, self.align, self.sentinel, self.name = int(nbytes), int(align), int(sentinel), name
        total = 2 * guard + self.nbytes + 2 * self.align
        if wrap is None:
            self.alloc = torch.empty(total, dtype=torch.uint8, device=device)
            self.base = self.alloc.data_ptr()
        else:
            import ctypes
            self.base, length = int(wrap[0]), int(wrap[1])
            assert length >= total, f"{name}: wrapping {length} bytes, {total} needed (GuardedBytes.wrapped_bytes)"
            self._keep = (ctypes.c_uint8 * length).from_address(self.base)
            self.alloc = torch.frombuffer(self._keep, dtype=torch.uint8)
        first = self.base + guard
        start = (first + self.align - 1) // self.align * self.align
        if start % (2 * self.align) == 0:
            start += self.align
        self.start = start - self.base                       # body offset inside the allocation
        assert self.start >= guard and self.start + self.nbytes + guard <= self.alloc.numel()
        self.alloc.fill_(self.sentinel)
        self.mask = None
        if mask is not None:
            self.mask = torch.as_tensor(mask, dtype=torch.bool).reshape(-1).to(self.alloc.device)
            assert self.mask.numel() == self.nbytes

    @staticmethod
    def wrapped_bytes(nbytes, align=256, guard=GUARD_BYTES):
        """Bytes a caller must own to wrap a body of nbytes (wrap=...)."""
        return 2 * guard + int(nbytes) + 2 * int(align)

    @property
    def ptr(self):
        return self.base + self.start

    @property
    def body(self):
        """The body as a uint8 tensor (a view of the allocation)."""
        return self.alloc[self.start:self.start + self.nbytes]

    def typed(self, dtype, shape=None):
        """The body, or its leading bytes, as a tensor of `dtype` (a view: writing through it initialises an in-out buffer)."""
        item = torch.empty(0, dtype=dtype).element_size()
        n = self.nbytes // item if shape is None else math.prod(shape)
        t = self.body[:n * item].view(dtype)
        return t if shape is None else t.reshape(shape)

    def result(self, dtype, shape=None):
        """A CPU copy of typed()."""
        return self.typed(dtype, shape).detach().cpu().clone()

    def refill(self):
        self.alloc.fill_(self.sentinel)

    def where(self, byte):
        """Offset of one byte of the allocation as the kernel addresses it (relative to the body pointer)."""
        k = int(byte) - self.start
        if k < 0:
            return f"guard before (byte {k})"
        if k >= self.nbytes:
            return f"guard after (byte {k - self.nbytes} past the end)"
        return f"body byte {k}"

    def _allowed(self, mask=None):
        m = torch.zeros(self.alloc.numel(), dtype=torch.bool, device=self.alloc.device)
        mask = self.mask if mask is None else torch.as_tensor(mask, dtype=torch.bool).reshape(-1).to(m.device)
        if mask is None:
            m[self.start:self.start + self.nbytes] = True
        else:
            assert mask.numel() == self.nbytes
            m[self.start:self.start + self.nbytes] = mask
        return m

    def verdict(self, mask=None):
        """-> (ok, message).  ok: every byte outside the allowed body bytes (`mask`, else the constructor's, else the whole body) still holds the sentinel."""
        bad = (self.alloc != self.sentinel) & ~self._allowed(mask)
        n = int(bad.sum())
        if n == 0:
            return True, f"{self.name}: nothing outside the declared bytes was written"
        idx = torch.nonzero(bad).reshape(-1)
        return False, (f"{self.name}: {n} byte(s) outside the declared bytes were written; first at {self.where(idx[0])}, last at {self.where(idx[-1])} "
                       f"(body of {self.nbytes} bytes at alignment {self.align})")

    def untouched(self):
        return bool((self.alloc == self.sentinel).all())

    def unwritten(self, mask=None):
        """Allowed body bytes that still hold the sentinel."""
        a = self._allowed(mask)
        return int(((self.alloc == self.sentinel) & a).sum())


# ------------------------------------------------------------------------------------------------------- logical [N, C, H, W] views of wider storage
POISONS = {"inf": float("inf"), "nan": float("nan"), "big": 3.0e38}
VIEW_GUARD = 4096             # floats of poison before and after the storage (a multiple of 64: the storage keeps the allocation's alignment)
VIEW_LAYOUTS = ("nchw", "nhwc", "nhwc_wide", "nhwc_off1", "nhwc_off2", "nhwc_ld3", "nchw_window", "nchw_window_odd", "batch_slice", "batch_slice_nchw",
                "batch_every_other", "batch_every_other_nchw", "every_other_pixel_nchw", "every_other_pixel_nhwc", "every_other_channel")


class StridedView:
    """A logical [N, C, H, W] fp32 tensor inside a larger allocation filled with `poison` ("inf", "nan", "big" or a float):

        nchw, nhwc                      packed (the controls)
        nhwc_wide                       [N, H, W, ld], channels [4, 4 + C), ld = C + 12
        nhwc_off1                       channels [1, 1 + C), ld = C + 7             (base only 4-byte aligned)
        nhwc_off2                       channels [2, 2 + C), ld = C + 6             (base 8-byte aligned, ld % 4 == 2 where C % 4 == 0)
        nhwc_ld3                        channels [3, 3 + C), ld = C + 3
        nhwc+OFF+PAD                    channels [OFF, OFF + C), ld = C + PAD       (any other slice, e.g. "nhwc+4+6")
        nchw_window                     [N, C, H + 3, W + 8], window at row 1, column 4
        nchw_window_odd                 [N, C, H + 3, W + 5], window at row 1, column 1
        batch_slice[_nchw]              images 1 .. N of N + 2                       (NHWC storage; _nchw: NCHW storage)
        batch_every_other[_nchw]        every other image of 2 N
        every_other_pixel_nchw / _nhwc  [:, :, ::2, ::2] of a 2H x 2W map
        every_other_channel             [:, ::2] of 2 C channels, NHWC storage       (channel stride 2: not channel-minor, every other stride % 4 == 0 where C % 2 == 0)

    .ptr / .strides (elements, logical n, c, y, x) are what a kernel is handed, .view the same as a torch view, .unchanged() whether the WHOLE allocation
    still holds the bits it was built with."""

    def __init__(self, data, layout, poison="nan", device="cpu", name="x"):
        N, C, H, W = (int(v) for v in data.shape)
        self.layout, self.name = layout, name
        p = POISONS[poison] if isinstance(poison, str) else float(poison)
        nhwc = lambda n, h, w, c: ((n, h, w, c), (0, 3, 1, 2))
        nchw = lambda n, c, h, w: ((n, c, h, w), (0, 1, 2, 3))
        sl = [slice(None)] * 4                                # slices in LOGICAL (n, c, y, x) order
        if layout == "nchw":
            shape, perm = nchw(N, C, H, W)
        elif layout == "nhwc":
            shape, perm = nhwc(N, H, W, C)
        elif layout in ("nhwc_wide", "nhwc_off1", "nhwc_off2", "nhwc_ld3") or layout.startswith("nhwc+"):
            if layout.startswith("nhwc+"):
                off, pad = (int(v) for v in layout.split("+")[1:])
                assert 0 <= off <= pad
            else:
                off, pad = {"nhwc_wide": (4, 12), "nhwc_off1": (1, 7), "nhwc_off2": (2, 6), "nhwc_ld3": (3, 3)}[layout]
            shape, perm = nhwc(N, H, W, C + pad)
            sl[1] = slice(off, off + C)
        elif layout == "nchw_window":
            shape, perm = nchw(N, C, H + 3, W + 8)
            sl[2], sl[3] = slice(1, H + 1), slice(4, W + 4)
        elif layout == "nchw_window_odd":
            shape, perm = nchw(N, C, H + 3, W + 5)
            sl[2], sl[3] = slice(1, H + 1), slice(1, W + 1)
        elif layout in ("batch_slice", "batch_slice_nchw"):
            shape, perm = (nchw(N + 2, C, H, W) if layout.endswith("nchw") else nhwc(N + 2, H, W, C))
            sl[0] = slice(1, N + 1)
        elif layout in ("batch_every_other", "batch_every_other_nchw"):
            shape, perm = (nchw(2 * N, C, H, W) if layout.endswith("nchw") else nhwc(2 * N, H, W, C))
            sl[0] = slice(0, 2 * N, 2)
        elif layout in ("every_other_pixel_nchw", "every_other_pixel_nhwc"):
            shape, perm = (nchw(N, C, 2 * H, 2 * W) if layout.endswith("nchw") else nhwc(N, 2 * H, 2 * W, C))
            sl[2], sl[3] = slice(0, 2 * H, 2), slice(0, 2 * W, 2)
        elif layout == "every_other_channel":
            shape, perm = nhwc(N, H, W, 2 * C)
            sl[1] = slice(0, 2 * C, 2)
        else:
            raise ValueError(layout)
        n = math.prod(shape)
        self.alloc = torch.full((2 * VIEW_GUARD + n,), p, dtype=torch.float32, device=device)
        storage = self.alloc[VIEW_GUARD:VIEW_GUARD + n].view(shape)
        self.view = storage.permute(perm)[tuple(sl)]
        assert tuple(self.view.shape) == (N, C, H, W)
        self.view.copy_(data.to(device=device, dtype=torch.float32))
        self.snapshot = self.alloc.clone()

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def strides(self):
        return tuple(int(s) for s in self.view.stride())

    @property
    def packed(self):
        return self.layout in ("nchw", "nhwc")

    def unchanged(self):
        return bool((self.alloc.view(torch.int32) == self.snapshot.view(torch.int32)).all())
