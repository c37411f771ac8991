"""GPU: every entry point of the C ABI that takes a pixel stride, run on channel SLICES of wider, guarded buffers (tests/strided_io.py).

The kernel-level tests elsewhere use packed, exactly sized outputs and read back only those elements: a store one pixel, one tile row or one 16-byte
vector past the ragged edge lands in allocator slack and nothing notices.  Here each launch runs twice on the same logical operands — packed, and as
slices at a nonzero channel offset with ldx, ldy and ldr all different — and must
  1. leave every int32 word outside its output slice (and outside every auxiliary output: splitk_scratch, fuse_part, the y_absmax slots) untouched;
  2. give bit for bit the packed result wherever the dispatcher reports the same kernel for both launches;
  3. satisfy the per-element float64 criterion of tests/test_gpu_plan_replay.py (_conv_parts / _den / _worst, R_CLASS of the class that RAN): no new
     tolerance; the elementwise entries go through that file's Checker itself;
  4. where a stride or an alignment sends the launch to another kernel (ldy % 4 != 0 or a y that is only 4-byte aligned: the row-Winograd kernels
     9 / 10 / 11 / 13 give way to 2 / 5 / 6), report a variant whose eligibility rule admits the launch;
  5. under CNL_ALGO_FORCE + v on a layout v cannot take, run another variant correctly (include/centernet_gfx950.h, CNL_ALGO_FORCE) — except a launch
     with fuse_w, which fails with CNL_E_UNSUPPORTED and leaves y untouched;
  6. report y_absmax == max |y| over the slice per image, exactly;
  7. let no NaN of the poisoned padding of x / residual reach the slice.
A stride or offset a launcher rejects must be REJECTED (return code, y all sentinel), never skipped.  The last test checks that the (entry, form) pairs
that ran under a strided layout cover the whole list."""
import ctypes
import functools
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

import test_gpu_plan_replay as rp
from centernet_lightning_amd import _lib, engine, params as P
from centernet_lightning_amd._lib import (CNL_ALGO_AUTO, CNL_ALGO_F32, CNL_ALGO_F43, CNL_ALGO_FORCE, CNL_E_BAD_ARG, CNL_E_UNSUPPORTED, CNL_RELU,
                                          CNL_RELU6, CNL_SIGMOID, CNL_UPSAMPLE_IN, CNL_UPSAMPLE_OUT_ADD, CNL_W_SPLIT, ConvParams, DeconvParams)
from strided_io import Guarded

pytestmark = pytest.mark.gpu
RAN = set()                 # (entry, form) pairs that ran under a strided layout

# (channel offset, ld - C) of x, y and the residual.  ldx % 4 == 0 always (every launcher asks for it); "wide" keeps everything 16-byte aligned.
LAYOUTS = {
    "packed": NS(x=(0, 0), y=(0, 0), r=(0, 0)),
    "wide": NS(x=(4, 12), y=(4, 4), r=(4, 8)),              # ldy % 4 == 0, y and residual 16-byte aligned
    "ldy3": NS(x=(4, 4), y=(3, 3), r=(4, 12)),              # ldy % 4 != 0 and y only 4-byte aligned
    "yoff3": NS(x=(4, 12), y=(3, 4), r=(4, 8)),             # ldy % 4 == 0 but y only 4-byte aligned
    "ldr3": NS(x=(4, 12), y=(4, 4), r=(3, 3)),              # ldr % 4 != 0, residual only 4-byte aligned
    "y0": NS(x=(0, 4), y=(0, 12), r=(0, 8)),                # offset 0, padding behind the slice only
}
ROW = (9, 10, 11, 13)
WINO_CLASS = {2: "wino_f32", 5: "wino_split", 6: "wino_split", 9: "row_wino", 10: "row_wino", 11: "row_wino", 13: "f43"}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _slot_only():
    only = torch.zeros(_lib.absmax_stride(), dtype=torch.bool)
    only[0] = True
    return only


def _slots(N):
    """A guarded y_absmax array: zeroed slots (the producer folds into them with an atomic max), sentinel between and around them."""
    g = Guarded((N,), _lib.absmax_stride(), device="cuda", name="y_absmax")
    g.view[:, 0] = 0.0
    return g


def _slot_values(g):
    return g.view[:, 0].cpu()


def _g(lead, C, lay, data=None, name="y"):
    off, add = lay
    return Guarded(lead, C, C + add, off, data=data, device="cuda", name=name)


# ---------------------------------------------------------------------------------------------------------------------------- conv-like entries
def spec(N, Cin, H, W, Cout, k=3, stride=1, flags=0, res=False, hints=False, presplit=False, splitk=0, algo=CNL_ALGO_AUTO, hand=True, w_up=False,
         fuse_c2=0, seed=0):
    """One logical launch of cnl_conv2d_nhwc_f32 / cnl_conv3x3_winograd_f32 / cnl_conv3x3_up2_nhwc_f32.  hints: x_absmax (+ w_absmax) handed over;
    hand (Winograd): x_absmax handed over instead of the kernel's own pass; fuse_c2: channels of a folded 1x1 conv (fuse_w / fuse_part)."""
    return NS(**locals())


@functools.lru_cache(maxsize=None)
def _operands(N, Cin, H, W, Cout, k, stride, out_add, up_in, res, seed):
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + H + W + k + seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    x[N - 1] *= 29.0                                            # images of different magnitude: scales and maxima are per image
    w = torch.randn(Cout, Cin, k, k, generator=g) * (1.0 / (Cin * k * k)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    up = 2 if up_in else 1
    ho, wo = (H * up + 2 * ((k - 1) // 2) - k) // stride + 1, (W * up + 2 * ((k - 1) // 2) - k) // stride + 1
    if out_add:
        ho, wo = 2 * ho, 2 * wo
    r = torch.randn(N, Cout, ho, wo, generator=g) if res else None
    return NS(x=x, w=w, b=b, r=r, ho=ho, wo=wo, wd=w.permute(0, 2, 3, 1).contiguous().cuda(), bd=b.cuda(), cache={})


def operands(s):
    return _operands(s.N, s.Cin, s.H, s.W, s.Cout, s.k, s.stride, bool(s.flags & CNL_UPSAMPLE_OUT_ADD), bool(s.flags & CNL_UPSAMPLE_IN), s.res, s.seed)


def f64_worst(s, ops, y_nhwc, cls):
    """max ratio |y - y64| / (u s + floor) of one result under the criterion of the arithmetic class that ran."""
    key = (rp.WINDOW.get(cls), cls in rp.SPLIT_CLASSES, s.flags & (CNL_RELU | CNL_RELU6 | CNL_SIGMOID))
    if key not in ops.cache:
        R = ops.r.double() if ops.r is not None else None
        z, sc, fl = rp._conv_parts(ops.x.double(), ops.w.double(), ops.b.double(), s.stride, (s.k - 1) // 2, s.flags, R, key[0], key[1])
        y64 = rp._act(z, s.flags)
        ops.cache[key] = (y64, rp._den(z, y64, sc, fl, s.flags))
    y64, den = ops.cache[key]
    return rp._worst(rp._nchw(y_nhwc), y64, den)


def _weights(entry, s, ops):
    """The weight buffer the entry reads (cached per logical launch: independent of the layout)."""
    lib = _lib.load()
    key = ("w", entry, s.presplit, s.w_up, s.fuse_c2)
    if key in ops.cache:
        return ops.cache[key]
    wd = ops.wd
    out = NS(w=None, w_up=None, fuse_w=None, wmax=wd.abs().max().reshape(1).contiguous(), out_w=None, out_b=None)
    if entry == "conv2d":
        out.w = wd
        if s.presplit:
            out.w = torch.full((lib.cnl_conv_split_weight_floats(s.Cin, s.Cout, s.k, s.k),), float("nan"), device="cuda")
            _lib.check(lib.cnl_conv_split_weights_f32(wd.data_ptr(), out.w.data_ptr(), s.Cin, s.Cout, s.k, s.k, _stream()), "split weights")
    elif entry == "winograd":
        out.w = torch.full((lib.cnl_winograd_weight_floats(s.Cin, s.Cout),), float("nan"), device="cuda")
        _lib.check(lib.cnl_winograd_transform_weights_f32(wd.data_ptr(), out.w.data_ptr(), s.Cin, s.Cout, _stream()), "winograd weights")
        if s.w_up:
            out.w_up = torch.full((lib.cnl_winograd_up_weight_floats(s.Cin, s.Cout),), float("nan"), device="cuda")
            _lib.check(lib.cnl_winograd_transform_weights_up_f32(wd.data_ptr(), out.w_up.data_ptr(), s.Cin, s.Cout, _stream()), "row-pair weights")
        if s.fuse_c2:
            g = torch.Generator().manual_seed(s.fuse_c2)
            out.out_w = torch.randn(s.fuse_c2, s.Cout, generator=g) * (1.0 / s.Cout) ** 0.5
            out.out_b = torch.randn(s.fuse_c2, generator=g) * 0.1
            out.fuse_w = torch.full(((s.Cout + 63) // 64 * 64 * 4,), float("nan"), device="cuda")
            _lib.check(lib.cnl_fused_out_pack_weights_f32(out.out_w.cuda().data_ptr(), out.fuse_w.data_ptr(), s.Cout, s.fuse_c2, _stream()), "fuse_w")
    else:
        out.w = torch.full((lib.cnl_up2_weight_floats(s.Cin, s.Cout),), float("nan"), device="cuda")
        _lib.check(lib.cnl_up2_pack_weights_f32(wd.data_ptr(), out.w.data_ptr(), s.Cin, s.Cout, _stream()), "up2 weights")
    torch.cuda.synchronize()
    ops.cache[key] = out
    return out


def run(entry, s, lay):
    """One launch of `entry` under layout `lay` -> rc, the slice, the kernel / variant the dispatcher reports, y_absmax, and the harness verdicts."""
    lib = _lib.load()
    ops = operands(s)
    wt = _weights(entry, s, ops)
    N = s.N
    x = _g((N, s.H, s.W), s.Cin, lay.x, ops.x.permute(0, 2, 3, 1), "x")
    y = _g((N, ops.ho, ops.wo), s.Cout, lay.y)
    r = _g((N, ops.ho, ops.wo), s.Cout, lay.r, ops.r.permute(0, 2, 3, 1), "residual") if s.res else None
    p = ConvParams()
    p.x, p.w, p.bias, p.y = x.ptr, wt.w.data_ptr(), ops.bd.data_ptr(), y.ptr
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, s.H, s.W, s.Cin, s.Cout
    p.KH = p.KW = s.k
    p.stride, p.pad, p.ldx, p.ldy, p.flags, p.algo = s.stride, (s.k - 1) // 2, x.ld, y.ld, s.flags, s.algo
    if r is not None:
        p.residual, p.ldr = r.ptr, r.ld
    aux = {}
    xm = _lib.absmax_pack(ops.x.abs().amax(dim=(1, 2, 3)).cuda())
    ym = _slots(N)
    aux["y_absmax"] = ym
    if entry == "conv2d":
        if s.presplit:
            p.flags |= CNL_W_SPLIT
        if s.hints:
            p.x_absmax, p.w_absmax = xm.data_ptr(), wt.wmax.data_ptr()
        p.y_absmax = ym.ptr
        if s.splitk:
            p.splitk = s.splitk
            nbytes = lib.cnl_conv2d_splitk_scratch_bytes(ctypes.byref(p))
            assert nbytes == s.splitk * N * ops.ho * ops.wo * s.Cout * 4
            aux["splitk_scratch"] = Guarded((s.splitk * N * ops.ho * ops.wo,), s.Cout, device="cuda", name="splitk_scratch")
            p.splitk_scratch, p.splitk_scratch_bytes = aux["splitk_scratch"].ptr, nbytes
        fn, kernel = lib.cnl_conv2d_nhwc_f32, lib.cnl_conv2d_kernel(ctypes.byref(p))
    elif entry == "winograd":
        if s.hand:
            p.x_absmax = xm.data_ptr()
        p.y_absmax = ym.ptr
        if s.w_up:
            p.w_up = wt.w_up.data_ptr()
        if s.fuse_c2:
            nb = (s.Cout + 63) // 64 * 2
            aux["fuse_part"] = Guarded((nb * N * ops.ho * ops.wo,), 4, device="cuda", name="fuse_part")
            p.fuse_w, p.fuse_part = wt.fuse_w.data_ptr(), aux["fuse_part"].ptr
        fn, kernel = lib.cnl_conv3x3_winograd_f32, lib.cnl_conv3x3_winograd_variant(ctypes.byref(p))
    else:
        if s.hints:
            p.x_absmax = xm.data_ptr()
        p.y_absmax = ym.ptr
        fn, kernel = lib.cnl_conv3x3_up2_nhwc_f32, lib.cnl_conv3x3_up2_kernel(ctypes.byref(p))
    rc = fn(ctypes.byref(p), _stream())
    torch.cuda.synchronize()
    bad = [msg for ok, msg in [y.verdict()] + [g.verdict(_slot_only() if k == "y_absmax" else None) for k, g in aux.items()] if not ok]
    if not x.unchanged() or (r is not None and not r.unchanged()):
        bad.append("an input buffer was written")
    return NS(rc=rc, y=y.result(), kernel=kernel, ymax=_slot_values(ym), bad=bad, yg=y, rg=r, xg=x, aux=aux, p=p, wt=wt,
              err=_lib.last_error() if rc else "")


def conv_class(entry, s, o):
    if entry == "conv2d":
        return "direct_split" if o.kernel == 5 else "direct_f32"
    if entry == "up2":
        return "subpixel_split" if o.kernel == 5 else "subpixel_f32"
    return WINO_CLASS[o.kernel]


def honours_ymax(entry, s, o):
    """include/centernet_gfx950.h, y_absmax: the fp16-split kernels and cnl_conv2d_nhwc_f32's CNL_UPSAMPLE_OUT_ADD epilogue."""
    if entry == "winograd":
        return o.kernel != 2
    return o.kernel == 5 or bool(s.flags & CNL_UPSAMPLE_OUT_ADD)


def assert_good(entry, s, o, what):
    """Checks 1, 3, 6, 7 of one launch that ran."""
    assert o.rc == 0, (what, o.rc, o.err)
    assert not o.bad, (what, o.bad)                                                        # 1
    assert o.yg.unwritten() == 0 and not torch.isnan(o.y).any(), (what, "sentinel / NaN inside the slice", o.yg.unwritten())      # 7
    cls = conv_class(entry, s, o)
    ratio, where = f64_worst(s, operands(s), o.y, cls)
    print(f"    {what}: kernel {o.kernel} class {cls} ratio {ratio:.3f} (R_CLASS {rp.R_CLASS[cls]})")
    assert ratio <= rp.R_CLASS[cls], (what, cls, ratio, where)                             # 3
    if honours_ymax(entry, s, o):
        assert torch.equal(o.ymax, o.y.abs().amax(dim=(1, 2, 3))), (what, o.ymax, o.y.abs().amax(dim=(1, 2, 3)))      # 6


def check(entry, s, layouts, form):
    """The packed launch, then each strided layout: checks 1 - 3, 6, 7.  `form`: name of the pair recorded in RAN, or a function of the result."""
    base = run(entry, s, LAYOUTS["packed"])
    assert_good(entry, s, base, f"{entry} packed")
    outs = {}
    for name in layouts:
        o = run(entry, s, LAYOUTS[name])
        assert_good(entry, s, o, f"{entry} {name}")
        if o.kernel == base.kernel:
            assert torch.equal(o.y, base.y), (entry, name, "the strided result differs from the packed one", o.kernel)         # 2
            if "fuse_part" in o.aux:
                assert torch.equal(o.aux["fuse_part"].result(), base.aux["fuse_part"].result()), (entry, name, "fuse_part differs")
        RAN.add((entry, form(o) if callable(form) else form))
        outs[name] = o
    return base, outs


def expect_reject(entry, s, layout, code):
    o = run(entry, s, LAYOUTS[layout] if isinstance(layout, str) else layout)
    assert o.rc == code, (entry, layout, o.rc, o.err)
    assert o.yg.untouched() and all(g.verdict(_slot_only() if k == "y_absmax" else None)[0] for k, g in o.aux.items()), (entry, layout, "a rejected launch wrote")
    if "fuse_part" in o.aux:
        assert o.aux["fuse_part"].untouched()


# ---- cnl_conv2d_nhwc_f32
DIRECT = [
    ("fp32 1x1", spec(2, 64, 5, 7, 20, k=1)),
    ("fp32 1x1 stride 2", spec(2, 64, 5, 7, 64, k=1, stride=2)),
    ("fp32 3x3", spec(3, 32, 9, 11, 130)),
    ("fp32 3x3 stride 2", spec(3, 32, 9, 11, 80, stride=2)),
    ("fp32 3x3 Cout 4", spec(2, 32, 5, 7, 4)),
    ("fp16-split 3x3", spec(3, 32, 9, 11, 130, hints=True)),
    ("fp16-split 3x3 stride 2", spec(3, 64, 9, 11, 80, stride=2, hints=True, flags=CNL_RELU)),
    ("fp16-split 1x1", spec(2, 64, 5, 7, 80, k=1, hints=True, algo=CNL_ALGO_FORCE + 5)),
    ("fp16-split 3x3, pre-split weights", spec(3, 32, 9, 11, 20, hints=True, presplit=True)),
    ("fp16-split 1x1, pre-split weights", spec(2, 64, 5, 7, 130, k=1, hints=True, presplit=True, algo=CNL_ALGO_FORCE + 5)),
    ("split-K 4", spec(2, 64, 5, 7, 130, hints=True, splitk=4, res=True, flags=CNL_RELU)),
    ("split-K 7", spec(3, 64, 9, 11, 20, hints=True, splitk=7, res=True, flags=CNL_RELU)),
    ("split-K 2 1x1", spec(2, 128, 5, 7, 64, k=1, hints=True, splitk=2)),
    ("upsample_in", spec(2, 32, 5, 7, 20, flags=CNL_RELU | CNL_UPSAMPLE_IN)),
    ("upsample_in Cout 130", spec(2, 64, 5, 7, 130, flags=CNL_UPSAMPLE_IN)),
    ("sigmoid", spec(2, 64, 5, 7, 80, k=1, flags=CNL_SIGMOID)),
    ("sigmoid fp16-split", spec(2, 64, 5, 7, 80, k=1, flags=CNL_SIGMOID, hints=True, algo=CNL_ALGO_FORCE + 5)),
    ("residual + relu", spec(3, 32, 9, 11, 20, res=True, flags=CNL_RELU)),
    ("residual + relu fp16-split", spec(3, 32, 9, 11, 64, res=True, flags=CNL_RELU, hints=True)),
]
@pytest.mark.parametrize("form,s", DIRECT, ids=[d[0] for d in DIRECT])
def test_conv2d_writes_only_its_slice(form, s):
    base, outs = check("conv2d", s, ["wide", "ldy3", "yoff3", "y0"] + (["ldr3"] if s.res else []), form)
    want = 5 if s.hints else 2
    assert base.kernel == want and all(o.kernel == want for o in outs.values()), (form, base.kernel)        # the direct kernels do not look at ldy / alignment
    if s.splitk:
        for o in outs.values():
            assert o.aux["splitk_scratch"].unwritten() < o.aux["splitk_scratch"].P * s.Cout               # the reduce form ran: slices were written


OUT_ADD = [spec(2, 64, 5, 7, 20, k=1, res=True, flags=CNL_UPSAMPLE_OUT_ADD), spec(3, 32, 9, 11, 80, k=1, res=True, flags=CNL_UPSAMPLE_OUT_ADD | CNL_RELU),
           spec(2, 64, 5, 7, 130, k=1, res=True, flags=CNL_UPSAMPLE_OUT_ADD)]


@pytest.mark.parametrize("s", OUT_ADD, ids=lambda s: f"N{s.N}c{s.Cin}_{s.H}x{s.W}_o{s.Cout}")
def test_conv2d_upsample_out_add_on_both_sides_of_the_vector_epilogue(s):
    """CNL_UPSAMPLE_OUT_ADD: the 16-byte epilogue (Cout, ldy, ldr multiples of 4, y and residual 16-byte aligned: "wide") and the scalar one (any of them
    not) are the same additions in the same order: every layout gives the packed launch's bits."""
    vec = lambda o: s.Cout % 4 == 0 and o.yg.ld % 4 == 0 and o.rg.ld % 4 == 0 and o.yg.aligned16 and o.rg.aligned16
    check("conv2d", s, ["wide", "ldy3", "yoff3", "ldr3", "y0"], lambda o: "out_add, 16-byte epilogue" if vec(o) else "out_add, scalar epilogue")


def test_conv2d_rejects_the_strides_its_header_excludes():
    s = spec(2, 32, 5, 7, 20, res=True)
    expect_reject("conv2d", s, NS(x=(0, 3), y=(0, 0), r=(0, 0)), CNL_E_BAD_ARG)         # ldx % 4 != 0
    expect_reject("conv2d", s, NS(x=(3, 4), y=(0, 0), r=(0, 0)), CNL_E_BAD_ARG)         # x only 4-byte aligned
    expect_reject("winograd", s, NS(x=(0, 3), y=(0, 0), r=(0, 0)), CNL_E_UNSUPPORTED)
    expect_reject("winograd", s, NS(x=(3, 4), y=(0, 0), r=(0, 0)), CNL_E_BAD_ARG)
    u = spec(2, 32, 5, 7, 20, flags=CNL_UPSAMPLE_IN)
    expect_reject("up2", u, NS(x=(0, 3), y=(0, 0), r=(0, 0)), CNL_E_BAD_ARG)
    expect_reject("up2", u, NS(x=(3, 4), y=(0, 0), r=(0, 0)), CNL_E_BAD_ARG)
    RAN.add(("conv2d", "rejections"))


# ---- cnl_conv3x3_winograd_f32
def admits(v, s, o):
    """The eligibility rules of the variants (csrc/winograd.hip wino_choice, cnl_wino9_eligible, cnl_wino13_eligible), restated."""
    y, r = o.yg, o.rg
    row = s.Cin % 32 == 0 and s.Cout % 4 == 0 and y.ld % 4 == 0 and y.aligned16 and (r is None or (r.ld % 4 == 0 and r.aligned16))
    if v in (9, 10, 11):
        return row
    if v == 13:
        return row and not (s.flags & CNL_UPSAMPLE_IN) and not s.fuse_c2
    if v == 6:
        return s.Cin % 16 == 0 and s.Cout % 128 == 0
    if v == 5:
        return s.Cin % 16 == 0
    return v == 2


def check_wino(s, layouts, tag=""):
    """check() + the variant rules: the reported variant admits the launch (4); a forced variant runs where the layout admits it, else another (5)."""
    forced = s.algo - CNL_ALGO_FORCE if s.algo >= CNL_ALGO_FORCE else None
    base, outs = check("winograd", s, layouts, lambda o: f"variant {o.kernel}{tag}" + (", default" if forced is None else ", forced"))
    for name, o in list(outs.items()) + [("packed", base)]:
        assert admits(o.kernel, s, o), (name, "the reported variant does not admit this launch", o.kernel)
        if forced is not None:
            if admits(forced, s, o):
                assert o.kernel == forced, (name, forced, o.kernel)
            else:
                assert o.kernel != forced, (name, forced)
                RAN.add(("winograd", f"forced {forced} on a layout it cannot take"))
        elif not all(admits(v, s, o) for v in ROW[:3]):
            assert o.kernel in (2, 5, 6), (name, o.kernel)
            RAN.add(("winograd", "alignment fallback to 2 / 5 / 6"))
        elif s.algo != CNL_ALGO_F32:                             # every shape of this file pads a row kernel's items by less than 1.5 x: the default is one of them
            assert o.kernel in ROW, (name, "the layout admits the row kernels, the default took", o.kernel)
    return base, outs


# N, Cin, H, W, Cout: row-kernel maps — packed rows (20, 34, 66), exact block rows (64, 128); heights whose 8- and 4-row items are both ragged
ROW_SHAPES = [(2, 32, 9, 20, 20), (3, 64, 19, 34, 80), (2, 32, 9, 66, 4), (2, 32, 19, 64, 64), (2, 32, 9, 128, 20)]


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda t: "N{}c{}_{}x{}_o{}".format(*t))
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_row_winograd_variants_write_only_their_slice(shape, res):
    """winograd9 / 10 / 11 (16-byte store epilogues, full-line stores, packed rows): default-chosen and forced, x_absmax handed over and the kernel's own
    pass; ldy % 4 != 0, a 4-byte aligned y or a misaligned residual send the launch to variants 2 / 5 / 6."""
    layouts = ["wide", "ldy3", "yoff3", "y0"] + (["ldr3"] if res else [])
    flags = CNL_RELU if res else 0
    base9, _ = check_wino(spec(*shape, res=res, flags=flags, algo=CNL_ALGO_FORCE + 9), layouts)
    for algo in (CNL_ALGO_AUTO, CNL_ALGO_FORCE + 10, CNL_ALGO_FORCE + 11):
        base, _ = check_wino(spec(*shape, res=res, flags=flags, algo=algo), layouts)
        if base.kernel in (9, 10, 11):
            assert torch.equal(base.y, base9.y), f"variant {base.kernel} is bit for bit winograd9"
    s = spec(*shape, res=res, flags=flags, algo=CNL_ALGO_FORCE + 32 + 9, hand=False)      # variant 9 on the plain block grid (no packed rows), the kernel's own max |x| pass
    o = run("winograd", s, LAYOUTS["wide"])
    assert_good("winograd", s, o, "winograd9 plain grid, own absmax pass")
    assert o.kernel == 9 and torch.equal(o.y, base9.y)
    RAN.add(("winograd", "variant 9, own absmax pass"))


@pytest.mark.parametrize("want,shape", [(9, (3, 32, 24, 64, 960)), (10, (5, 256, 9, 16, 260))], ids=["variant 9", "variant 10"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_row_winograd_9_and_10_as_the_dispatchers_own_choice(want, shape, res):
    """The two row variants the small maps above never get by default.  9: a plain launch of more than 128 of its 8-row x 64-cout items (3 x 3 block
    rows x 15 cout blocks = 135) on a height 8-row items do not pad.  10: 16-pixel-wide maps with Cin >= 256 and Cout > 256, whatever the grid — four
    images side by side in a block row, the fifth alone in the next.  Same checks, same fallbacks (2 / 5 / 6) under the layouts they cannot take."""
    s = spec(*shape, res=res, flags=CNL_RELU if res else 0)
    base, outs = check_wino(s, ["wide", "ldy3", "yoff3", "y0"] + (["ldr3"] if res else []))
    assert base.kernel == want and outs["wide"].kernel == want and outs["y0"].kernel == want, (want, base.kernel, outs["wide"].kernel)
    forced = run("winograd", spec(*shape, res=res, flags=s.flags, algo=CNL_ALGO_FORCE + 9), LAYOUTS["wide"])
    assert forced.kernel == 9 and torch.equal(forced.y, outs["wide"].y)


def test_row_winograd_excludes_cout_not_a_multiple_of_4():
    """Cout = 130: no row kernel, default or forced, under any layout (the 16-byte epilogue would straddle the slice's end)."""
    for algo in (CNL_ALGO_AUTO, CNL_ALGO_FORCE + 9, CNL_ALGO_FORCE + 11, CNL_ALGO_FORCE + 13):
        s = spec(2, 32, 9, 20, 130, algo=algo, res=True)
        base, outs = check_wino(s, ["wide", "y0"])
        assert base.kernel not in ROW and all(o.kernel not in ROW for o in outs.values())
    RAN.add(("winograd", "Cout % 4 != 0 excluded from the row kernels"))


F22 = [
    (2, spec(2, 24, 9, 20, 20, res=True, flags=CNL_RELU)),                               # Cin % 16 != 0: the fp32 kernel, whatever is asked
    (2, spec(2, 32, 7, 5, 130, algo=CNL_ALGO_F32)),
    (2, spec(3, 32, 9, 11, 20, algo=CNL_ALGO_FORCE + 2, res=True)),
    (5, spec(2, 128, 19, 34, 130, res=True, flags=CNL_RELU)),                            # Cout % 4 != 0: no row kernel; Cout % 128 != 0: 5
    (5, spec(2, 128, 19, 34, 80, algo=CNL_ALGO_FORCE + 5, hand=False)),
    (5, spec(2, 128, 9, 20, 64, algo=CNL_ALGO_FORCE + 6)),                               # 6 needs Cout % 128 == 0: runs 5
    (6, spec(2, 128, 19, 34, 128, algo=CNL_ALGO_FORCE + 6, res=True, flags=CNL_RELU)),
    (6, spec(3, 64, 9, 20, 256, algo=CNL_ALGO_FORCE + 6, hand=False)),
]


@pytest.mark.parametrize("want,s", F22, ids=[f"v{w}_N{s.N}c{s.Cin}_{s.H}x{s.W}_o{s.Cout}_a{s.algo}" for w, s in F22])
def test_f22_winograd_variants_write_only_their_slice(want, s):
    """winograd2 / 5 / 6 (element stores with per-element masks): any ldy, any alignment of y and the residual — the same variant and the same bits."""
    base, outs = check_wino(s, ["wide", "ldy3", "yoff3", "y0"] + (["ldr3"] if s.res else []))
    assert base.kernel == want and all(o.kernel == want for o in outs.values()), (want, base.kernel, [o.kernel for o in outs.values()])


def test_winograd6_is_the_default_where_the_layout_excludes_the_row_kernels():
    s = spec(2, 128, 19, 34, 128, res=True, flags=CNL_RELU)
    base, outs = check_wino(s, ["wide", "ldy3", "yoff3", "ldr3"])
    assert base.kernel in ROW and outs["wide"].kernel == base.kernel
    assert [outs[k].kernel for k in ("ldy3", "yoff3", "ldr3")] == [6, 6, 6]
    RAN.add(("winograd", "variant 6, default"))


@pytest.mark.parametrize("shape", [(2, 128, 9, 128, 64), (2, 128, 19, 132, 20)], ids=lambda t: "N{}c{}_{}x{}_o{}".format(*t))
def test_winograd13_writes_only_its_slice(shape):
    """F(4,3) along x (four 16-byte stores per lane and tile): CNL_ALGO_F43's choice on maps >= 128 wide, and forced; its fallbacks are 9, then 5."""
    for algo, res in ((CNL_ALGO_F43, False), (CNL_ALGO_F43, True), (CNL_ALGO_FORCE + 13, True)):
        s = spec(*shape, algo=algo, res=res, flags=CNL_RELU)
        base, outs = check_wino(s, ["wide", "ldy3", "yoff3", "y0"] + (["ldr3"] if res else []))
        assert base.kernel == 13 and outs["wide"].kernel == 13 and outs["y0"].kernel == 13, (algo, base.kernel)
    s = spec(2, 64, 9, 34, 20, algo=CNL_ALGO_FORCE + 13, flags=CNL_UPSAMPLE_IN)             # behind a folded upsample: 13 cannot, 9 can
    base, outs = check_wino(s, ["wide", "ldy3"])
    assert base.kernel == 9 and outs["ldy3"].kernel not in ROW
    s = spec(2, 64, 19, 66, 20, algo=CNL_ALGO_FORCE + 13, hand=False)                        # narrow maps: only when forced
    base, outs = check_wino(s, ["wide"])
    assert base.kernel == 13


@pytest.mark.parametrize("shape", [(2, 32, 5, 10, 20), (2, 64, 9, 17, 80), (3, 32, 4, 33, 64)], ids=lambda t: "N{}c{}_{}x{}_o{}".format(*t))
def test_winograd9_behind_a_folded_upsample(shape):
    """CNL_UPSAMPLE_IN: the general form and the row-pair form (w_up) — variant 9 by default (the half-height items have no folded upsample)."""
    for w_up in (False, True):
        s = spec(*shape, flags=CNL_RELU | CNL_UPSAMPLE_IN, w_up=w_up)
        base, outs = check_wino(s, ["wide", "ldy3", "y0"], tag=" + w_up" if w_up else " + upsample_in")
        assert base.kernel == 9 and outs["wide"].kernel == 9 and outs["ldy3"].kernel in (2, 5, 6)


REDUCE_LAYOUTS = {"vector": (4, 4), "ldy % 4 != 0": (3, 3), "y 4-byte aligned": (3, 4), "packed": (0, 0), "y0": (0, 12)}


@pytest.mark.parametrize("c2", [1, 2, 3, 4])
def test_winograd9_folded_out_conv_and_its_reduce(c2):
    """fuse_w / fuse_part (variant 9's epilogue) and cnl_fused_out_reduce_f32: the partial sums land in fuse_part only; the reduce writes C2 channels per
    pixel with one 16-byte store (C2 == 4, ldy % 4 == 0, y 16-byte aligned) or element by element — the same bits either way."""
    lib = _lib.load()
    chk = rp.Checker(NS(lib=lib, launches=[]), "strided")
    for shape in ((2, 32, 9, 20, 64), (3, 64, 19, 34, 80)):
        s = spec(*shape, flags=CNL_RELU, fuse_c2=c2)
        base, outs = check_wino(s, ["wide", "y0"], tag=" + fuse_w")
        assert base.kernel == 9 and all(o.kernel == 9 for o in outs.values())
        for lay in ("ldy3", "yoff3"):                            # a layout variant 9 cannot take: the fold is refused, nothing is written
            expect_reject("winograd", s, lay, CNL_E_UNSUPPORTED)
        RAN.add(("winograd", "fuse_w refused on a layout variant 9 cannot take"))
        o = outs["wide"]
        part = o.aux["fuse_part"]
        nb, M = (s.Cout + 63) // 64 * 2, s.N * s.H * s.W
        outl = NS(cout=c2, w=o.wt.out_w, b=o.wt.out_b)
        key = object()
        chk.out_of[id(key)] = outl
        L = NS(fn=lib.cnl_conv3x3_winograd_f32, args=o.p, keep=[None, None, None, None, key], what=f"winograd9 + fuse_w C2={c2}")
        chk._part(0, L, {"part": part.result().view(nb, M, 4), "y": o.y})
        bias = o.wt.out_b.cuda()
        got = {}
        for name, lay in REDUCE_LAYOUTS.items():
            for flags in (0, CNL_SIGMOID):
                y2 = _g((M,), c2, lay, name="reduce y")
                _lib.check(lib.cnl_fused_out_reduce_f32(part.ptr, nb, M, c2, bias.data_ptr(), y2.ptr, y2.ld, flags, _stream()), "reduce")
                torch.cuda.synchronize()
                ok, msg = y2.verdict()
                assert ok, (name, msg)
                assert y2.unwritten() == 0 and part.verdict()[0]
                got[(name, flags)] = y2.result()
                assert torch.equal(got[(name, flags)], got[("vector", flags)]), (name, flags)
                Lr = NS(fn=lib.cnl_fused_out_reduce_f32, args=(part.ptr, nb, M, c2, None, y2.ptr, y2.ld, flags), keep=[None, outl], what=f"reduce {name}")
                chk._reduce(1, Lr, {"part": part.result().view(nb, M, 4)}, {"y": got[(name, flags)]})
            vec = c2 == 4 and y2.ld % 4 == 0 and y2.aligned16
            if name != "packed":
                RAN.add(("fused_out_reduce", "16-byte store" if vec else "element stores"))
    assert not chk.fail, chk.report()


# ---- cnl_conv3x3_up2_nhwc_f32
@pytest.mark.parametrize("shape", [(2, 32, 5, 7, 20), (2, 64, 9, 11, 130), (3, 32, 4, 9, 64)], ids=lambda t: "N{}c{}_{}x{}_o{}".format(*t))
@pytest.mark.parametrize("hints", [False, True], ids=["fp32", "fp16-split"])
def test_subpixel_phases_write_only_their_slice(shape, hints):
    s = spec(*shape, flags=CNL_RELU | CNL_UPSAMPLE_IN, hints=hints)
    base, outs = check("up2", s, ["wide", "ldy3", "yoff3", "y0"], "fp16-split" if hints else "fp32")
    assert base.kernel == (5 if hints else 2) and all(o.kernel == base.kernel for o in outs.values())


# ---------------------------------------------------------------------------------------------------------------------------- cnl_pointwise_nhwc_f32
def _pointwise(N, H, W, C1, Cout, lay, C2=0, s2=1, odd=False, res=False, algo=0, lay2=(4, 12)):
    lib = _lib.load()
    g = torch.Generator().manual_seed(C1 + Cout + C2 + s2)
    x1 = torch.randn(N, H, W, C1, generator=g).clamp_min(0)
    x1[N - 1] *= 17.0
    H2, W2 = (H, W) if s2 == 1 else (2 * H - (1 if odd else 0), 2 * W - (1 if odd else 0))
    x2 = torch.randn(N, H2, W2, C2, generator=g).clamp_min(0) * 3.0 if C2 else None
    w = torch.randn(Cout, C1 + C2, generator=g) * (2.0 / (C1 + C2)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(N, H, W, Cout, generator=g) if res else None
    wd = w.contiguous().cuda()
    wbuf = torch.empty(lib.cnl_conv_split_weight_floats(C1 + C2, Cout, 1, 1), device="cuda")
    _lib.check(lib.cnl_conv_split_weights_f32(wd.data_ptr(), wbuf.data_ptr(), C1 + C2, Cout, 1, 1, _stream()), "split")
    xg = _g((N, H, W), C1, lay.x, x1, "x")
    yg = _g((N, H, W), Cout, lay.y)
    rg = _g((N, H, W), Cout, lay.r, r, "residual") if res else None
    x2g = _g((N, H2, W2), C2, lay2, x2, "x2") if C2 else None
    ym = _slots(N)
    xm1 = _lib.absmax_pack(x1.abs().amax(dim=(1, 2, 3)).cuda())
    xm2 = _lib.absmax_pack(x2.abs().amax(dim=(1, 2, 3)).cuda()) if C2 else None
    bd = b.cuda()
    p = ConvParams()
    p.x, p.w, p.bias, p.y = xg.ptr, wbuf.data_ptr(), bd.data_ptr(), yg.ptr
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, H, W, C1, Cout
    p.KH = p.KW = p.stride = 1
    p.ldx, p.ldy, p.flags, p.algo = xg.ld, yg.ld, CNL_RELU | CNL_W_SPLIT, algo
    if res:
        p.residual, p.ldr = rg.ptr, rg.ld
    p.x_absmax, p.y_absmax = xm1.data_ptr(), ym.ptr
    if C2:
        rc = lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), x2g.ptr, H2, W2, C2, x2g.ld, s2, xm2.data_ptr(), _stream())
    else:
        rc = lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), None, 0, 0, 0, 0, 1, None, _stream())
    torch.cuda.synchronize()
    if rc:
        return NS(rc=rc, yg=yg, ym=ym)
    ok, msg = yg.verdict()
    assert ok, msg
    ok, msg = ym.verdict(_slot_only())
    assert ok, msg
    assert xg.unchanged() and (rg is None or rg.unchanged()) and (x2g is None or x2g.unchanged())
    y = yg.result()
    assert yg.unwritten() == 0 and not torch.isnan(y).any()
    assert torch.equal(_slot_values(ym), y.abs().amax(dim=(1, 2, 3)))
    # float64, the per-element bound of the direct fp16-split class with the shared scale of the two sources (tests/test_gpu_bottleneck.py)
    w1, w2 = w[:, :C1].double(), w[:, C1:].double()
    z = x1.double().reshape(-1, C1) @ w1.t()
    sa = x1.double().abs().reshape(-1, C1) @ w1.abs().t()
    xsum = x1.double().abs().sum(-1, keepdim=True)
    xm = x1.abs().amax(dim=(1, 2, 3))
    if C2:
        xs = x2[:, ::s2, ::s2].double()
        z = z + xs.reshape(-1, C2) @ w2.t()
        sa = sa + xs.abs().reshape(-1, C2) @ w2.abs().t()
        xsum = xsum + xs.abs().sum(-1, keepdim=True)
        xm = torch.maximum(xm, x2.abs().amax(dim=(1, 2, 3)))
    z = z.reshape(N, H, W, Cout) + b.double()
    sa = sa.reshape(N, H, W, Cout) + b.double().abs()
    if res:
        z, sa = z + r.double(), sa + r.double().abs()
    floor = rp.FLOOR * (xm.double().view(-1, 1, 1, 1) * w.double().abs().sum(1) + float(w.abs().max()) * xsum)
    ratio, where = rp._worst(y, z.clamp_min(0), rp.U * sa + floor)
    assert ratio <= rp.R_CLASS["direct_split"], (ratio, where)
    return NS(rc=0, y=y, ratio=ratio)


@pytest.mark.parametrize("t", [0, 1, 2, 3], ids=["auto", "64x128", "128x128", "256x64"])
@pytest.mark.parametrize("cout", [20, 64, 130])
def test_pointwise_writes_only_its_slice(t, cout):
    """One source, two sources (ldx2 > C2, stride2 1 and 2, an odd H2 / W2), residual, every pinned tile shape: same bits as the packed launch."""
    algo = CNL_ALGO_FORCE + t if t else 0
    for kw in (dict(C1=32), dict(C1=64, res=True), dict(C1=32, C2=32, s2=1, res=True), dict(C1=64, C2=32, s2=2), dict(C1=32, C2=64, s2=2, odd=True, res=True)):
        base = _pointwise(3, 5, 7, Cout=cout, lay=LAYOUTS["packed"], algo=algo, lay2=(0, 0), **kw)
        assert base.rc == 0
        for name in ("wide", "ldy3", "yoff3", "y0") + (("ldr3",) if kw.get("res") else ()):
            o = _pointwise(3, 5, 7, Cout=cout, lay=LAYOUTS[name], algo=algo, **kw)
            assert o.rc == 0 and torch.equal(o.y, base.y), (name, kw)
        RAN.add(("pointwise", ("two sources, stride2 %d" % kw["s2"] if kw.get("C2") else "one source") + (", residual" if kw.get("res") else "")))
        RAN.add(("pointwise", f"tile shape {t}"))
    bad = _pointwise(3, 5, 7, C1=32, Cout=cout, lay=NS(x=(0, 3), y=(0, 0), r=(0, 0)), algo=algo)                 # ldx % 4 != 0
    assert bad.rc == CNL_E_BAD_ARG and bad.yg.untouched()
    bad = _pointwise(3, 5, 7, C1=32, C2=32, Cout=cout, lay=LAYOUTS["wide"], algo=algo, lay2=(0, 3))              # ldx2 % 4 != 0
    assert bad.rc == CNL_E_BAD_ARG and bad.yg.untouched()


# ---------------------------------------------------------------------------------------------------------------------------- the elementwise entries
def _shim():
    lib = _lib.load()
    return lib, rp.Checker(NS(lib=lib, launches=[]), "strided")


def _finish(chk, outs, ins):
    torch.cuda.synchronize()
    for gd in outs:
        ok, msg = gd.verdict()
        assert ok, msg
        assert gd.unwritten() == 0 and not torch.isnan(gd.result()).any(), gd.name
    assert all(gd.unchanged() for gd in ins if gd is not None)
    assert not chk.fail, chk.report()


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("cout", [20, 64, 130])
def test_deconv_writes_only_its_slice(K, cout):
    lib, chk = _shim()
    cin, N, H, W = 32, 2, 5, 7
    g = torch.Generator().manual_seed(K * 100 + cout)
    op = K % 2
    mod = P.DeconvBn(cin, K, init_bilinear=False)
    mod._modules["0"] = torch.nn.ConvTranspose2d(cin, cout, K, stride=2, padding=(K + op) // 2 - 1, output_padding=op, bias=False)
    mod._modules["1"] = torch.nn.BatchNorm2d(cout)
    with torch.no_grad():
        mod.deconv.weight.copy_(torch.randn(mod.deconv.weight.shape, generator=g) * 0.1)
        mod.bn.weight.copy_(torch.rand(cout, generator=g) + 0.5); mod.bn.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        mod.bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.2); mod.bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    mod.eval()
    layer = engine._DeconvLayer(mod, torch.device("cuda:0"))
    x = torch.randn(N, H, W, cin, generator=g)
    r = torch.randn(N, 2 * H, 2 * W, cout, generator=g)
    got = {}
    for name in ("packed", "wide", "ldy3", "yoff3", "ldr3", "y0"):
        lay = LAYOUTS[name]
        xg, yg, rg = _g((N, H, W), cin, lay.x, x, "x"), _g((N, 2 * H, 2 * W), cout, lay.y), _g((N, 2 * H, 2 * W), cout, lay.r, r, "residual")
        p = DeconvParams()
        p.x, p.w, p.bias, p.y, p.residual = xg.ptr, layer.w.data_ptr(), layer.b.data_ptr(), yg.ptr, rg.ptr
        p.N, p.H_in, p.W_in, p.Cin, p.Cout, p.K = N, H, W, cin, cout, K
        p.ldx, p.ldy, p.ldr, p.flags = xg.ld, yg.ld, rg.ld, CNL_RELU
        _lib.check(lib.cnl_deconv2x_nhwc_f32(ctypes.byref(p), _stream()), "deconv")
        L = NS(fn=lib.cnl_deconv2x_nhwc_f32, args=p, keep=[None, None, None, layer], what=f"deconv K={K} {name}")
        torch.cuda.synchronize()
        got[name] = yg.result()
        chk(0, L, {"x": x, "res": r}, {"y": got[name]})
        _finish(chk, [yg], [xg, rg])
        assert torch.equal(got[name], got["packed"]), name
    p.ldx = xg.ld + 3
    yg.refill()
    assert lib.cnl_deconv2x_nhwc_f32(ctypes.byref(p), _stream()) == CNL_E_BAD_ARG and yg.untouched()
    RAN.add(("deconv", f"K={K}"))


RESIZE_BAD = [NS(x=(0, 3), y=(0, 0), r=(0, 0)), NS(x=(0, 0), y=(0, 3), r=(0, 0)), NS(x=(0, 0), y=(0, 0), r=(0, 3))]          # a stride that is no multiple of 4
RESIZE_UNALIGNED = [NS(x=(3, 4), y=(0, 0), r=(0, 0)), NS(x=(0, 0), y=(3, 4), r=(0, 0)), NS(x=(0, 0), y=(0, 0), r=(3, 4))]    # a pointer that is only 4-byte aligned


@pytest.mark.parametrize("mode", [0, 1], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_upsample2x_writes_only_its_slice(mode, res):
    lib, chk = _shim()
    N, H, W, C = 3, 5, 7, 20
    g = torch.Generator().manual_seed(mode)
    x, r = torch.randn(N, H, W, C, generator=g), torch.randn(N, 2 * H, 2 * W, C, generator=g)
    got = {}

    def launch(lay):
        xg, yg, rg = _g((N, H, W), C, lay.x, x, "x"), _g((N, 2 * H, 2 * W), C, lay.y), _g((N, 2 * H, 2 * W), C, lay.r, r, "residual")
        args = (xg.ptr, rg.ptr if res else None, yg.ptr, N, H, W, C, xg.ld, rg.ld, yg.ld, mode)
        return lib.cnl_upsample2x_nhwc_f32(*args, _stream()), args, xg, yg, rg

    for name in ("packed", "wide", "y0"):
        rc, args, xg, yg, rg = launch(LAYOUTS[name])
        assert rc == 0
        torch.cuda.synchronize()
        got[name] = yg.result()
        chk(0, NS(fn=lib.cnl_upsample2x_nhwc_f32, args=args, keep=[], what=f"upsample2x {name}"), {"x": x, **({"res": r} if res else {})}, {"y": got[name]})
        _finish(chk, [yg], [xg, rg])
        assert torch.equal(got[name], got["packed"]), name
    for lay in RESIZE_BAD[:3 if res else 2]:
        rc, _, _, yg, _ = launch(lay)
        assert rc == CNL_E_UNSUPPORTED and yg.untouched(), lay
    for lay in RESIZE_UNALIGNED[:3 if res else 2]:
        rc, _, _, yg, _ = launch(lay)
        assert rc == CNL_E_BAD_ARG and yg.untouched(), lay
    RAN.add(("upsample2x", f"mode {mode}"))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("three", [False, True], ids=["two inputs", "three inputs"])
def test_fuse_sum_writes_only_its_slice(mode, three):
    lib, chk = _shim()
    N, H, W, C = 2, 6, 10, 20
    g = torch.Generator().manual_seed(10 * mode + three)
    lh, lw = {0: (H // 2, W // 2), 1: (H // 2, W // 2), 2: (2 * H, 2 * W), 3: (H, W)}[mode]
    a, b, last = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g), torch.randn(N, lh, lw, C, generator=g)
    for gains in ((1.0, 1.0, 1.0, 1.0), (0.75, 0.25 if three else 0.0, 1.5, 2.5 if three else 2.25)):
        got = {}
        for name, lays in (("packed", [(0, 0)] * 4), ("wide", [(4, 12), (4, 8), (8, 16), (4, 4)]), ("y0", [(0, 4), (0, 8), (0, 16), (0, 12)])):
            ag, bg, lg = _g((N, H, W), C, lays[0], a, "in0"), _g((N, H, W), C, lays[1], b, "in1"), _g((N, lh, lw), C, lays[2], last, "last")
            yg = _g((N, H, W), C, lays[3])
            args = (ag.ptr, bg.ptr if three else None, lg.ptr, yg.ptr, N, H, W, C, ag.ld, bg.ld, lg.ld, yg.ld) + gains + (mode,)
            _lib.check(lib.cnl_fuse_sum_nhwc_f32(*args, _stream()), "fuse_sum")
            torch.cuda.synchronize()
            got[name] = yg.result()
            chk(0, NS(fn=lib.cnl_fuse_sum_nhwc_f32, args=args, keep=[], what=f"fuse_sum {name}"),
                {"in0": a, "last": last, **({"in1": b} if three else {})}, {"y": got[name]})
            _finish(chk, [yg], [ag, bg, lg])
            assert torch.equal(got[name], got["packed"]), name
    for i in range(4):                                           # every stride a multiple of 4, every pointer 16-byte aligned: else refused, y untouched
        for lay, code in (((0, 3), CNL_E_UNSUPPORTED), ((3, 4), CNL_E_BAD_ARG)):
            if i == 1 and not three:
                continue
            lays = [(0, 0)] * 4
            lays[i] = lay
            ag, bg, lg = _g((N, H, W), C, lays[0], a, "in0"), _g((N, H, W), C, lays[1], b, "in1"), _g((N, lh, lw), C, lays[2], last, "last")
            yg = _g((N, H, W), C, lays[3])
            rc = lib.cnl_fuse_sum_nhwc_f32(ag.ptr, bg.ptr if three else None, lg.ptr, yg.ptr, N, H, W, C, ag.ld, bg.ld, lg.ld, yg.ld, 1.0, 1.0, 1.0, 1.0, mode, _stream())
            torch.cuda.synchronize()
            assert rc == code and yg.untouched(), (i, lay, rc)
    RAN.add(("fuse_sum", (mode, three)))


@pytest.mark.parametrize("shape,flags", [((2, 9, 11, 20), CNL_RELU6), ((3, 5, 7, 64), 0)])
def test_depthwise_writes_only_its_slice(shape, flags):
    lib, chk = _shim()
    N, H, W, C = shape
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, H, W, C, generator=g) * 3
    layer = NS(dw_w=(torch.randn(3, 3, C, generator=g)).cuda(), dw_b=torch.randn(C, generator=g).cuda())
    got = {}
    for name, lx, ly in (("packed", (0, 0), (0, 0)), ("wide", (4, 12), (4, 4)), ("y0", (0, 4), (0, 12))):
        xg, yg = _g((N, H, W), C, lx, x, "x"), _g((N, H, W), C, ly)
        args = (xg.ptr, layer.dw_w.data_ptr(), layer.dw_b.data_ptr(), yg.ptr, N, H, W, C, xg.ld, yg.ld, flags)
        _lib.check(lib.cnl_depthwise3x3_nhwc_f32(*args, _stream()), "depthwise")
        torch.cuda.synchronize()
        got[name] = yg.result()
        chk(0, NS(fn=lib.cnl_depthwise3x3_nhwc_f32, args=args, keep=[None, None, layer], what=f"depthwise {name}"), {"x": x}, {"y": got[name]})
        _finish(chk, [yg], [xg])
        assert torch.equal(got[name], got["packed"]), name
    for lx, ly, code in (((0, 3), (0, 0), CNL_E_UNSUPPORTED), ((0, 0), (0, 3), CNL_E_UNSUPPORTED), ((3, 4), (0, 0), CNL_E_BAD_ARG), ((0, 0), (3, 4), CNL_E_BAD_ARG)):
        xg, yg = _g((N, H, W), C, lx, x, "x"), _g((N, H, W), C, ly)
        rc = lib.cnl_depthwise3x3_nhwc_f32(xg.ptr, layer.dw_w.data_ptr(), layer.dw_b.data_ptr(), yg.ptr, N, H, W, C, xg.ld, yg.ld, flags, _stream())
        torch.cuda.synchronize()
        assert rc == code and yg.untouched(), (lx, ly, rc)
    RAN.add(("depthwise", "3x3"))


@pytest.mark.parametrize("K,has_mask", [(3, True), (3, False), (1, True)])
def test_deform_sample_writes_only_its_col(K, has_mask):
    """cnl_deform_sample_nhwc_f32: x a strided slice (ldx), the offsets / mask logits a strided slice with any stride (ldo: scalar loads), col packed
    [N, H, W, K K C] inside guards (the entry has no stride for it)."""
    lib, chk = _shim()
    N, H, W, C = 2, 5, 7, 20
    KK = K * K
    no = (3 if has_mask else 2) * KK
    g = torch.Generator().manual_seed(K + has_mask)
    x = torch.randn(N, H, W, C, generator=g)
    om = torch.cat([(torch.rand(N, H, W, 2 * KK, generator=g) - 0.5) * 5, torch.randn(N, H, W, no - 2 * KK, generator=g)], dim=-1)
    om[:, 0, 0, :2 * KK] = 0.0
    got = {}
    for name, lx, lo in (("packed", (0, 0), (0, 0)), ("wide", (4, 12), (3, 3)), ("y0", (0, 4), (0, 5))):
        xg, og, col = _g((N, H, W), C, lx, x, "x"), _g((N, H, W), no, lo, om, "om"), _g((N, H, W), KK * C, (0, 0), name="col")
        args = (xg.ptr, og.ptr, col.ptr, N, H, W, C, xg.ld, og.ld, K, int(has_mask))
        _lib.check(lib.cnl_deform_sample_nhwc_f32(*args, _stream()), "deform_sample")
        torch.cuda.synchronize()
        got[name] = col.result()
        shim_args = (xg.ptr, og.ptr, col.ptr, N, H, W, C, xg.ld, no, K, int(has_mask))
        chk(0, NS(fn=lib.cnl_deform_sample_nhwc_f32, args=shim_args, keep=[], what=f"deform_sample {name}"), {"x": x, "om": om}, {"y": got[name]})
        _finish(chk, [col], [xg, og])
        assert torch.equal(got[name], got["packed"]), name
    for lx, code in (((0, 3), CNL_E_UNSUPPORTED), ((3, 4), CNL_E_BAD_ARG)):
        xg, og, col = _g((N, H, W), C, lx, x, "x"), _g((N, H, W), no, (0, 0), om, "om"), _g((N, H, W), KK * C, (0, 0), name="col")
        rc = lib.cnl_deform_sample_nhwc_f32(xg.ptr, og.ptr, col.ptr, N, H, W, C, xg.ld, og.ld, K, int(has_mask), _stream())
        torch.cuda.synchronize()
        assert rc == code and col.untouched(), (lx, rc)
    RAN.add(("deform_sample", f"K={K} mask={has_mask}"))


# ---------------------------------------------------------------------------------------------------------------------------- entries without an output stride
@pytest.mark.parametrize("shape", [(2, 9, 11, 20), (3, 17, 23, 64), (2, 6, 6, 8)])
def test_maxpool_writes_only_its_output(shape):
    """cnl_maxpool3x3s2_nhwc_f32 takes no stride: packed tensors inside guards, bit-exact."""
    lib = _lib.load()
    N, H, W, C = shape
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(2))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xg, yg = _g((N, H, W), C, (0, 0), x, "x"), _g((N, Ho, Wo), C, (0, 0))
    _lib.check(lib.cnl_maxpool3x3s2_nhwc_f32(xg.ptr, yg.ptr, N, H, W, C, _stream()), "maxpool")
    torch.cuda.synchronize()
    ok, msg = yg.verdict()
    assert ok, msg
    assert xg.unchanged() and torch.equal(yg.result().permute(0, 3, 1, 2), F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1))
    bad = _g((N, Ho, Wo), C, (3, 4))
    assert lib.cnl_maxpool3x3s2_nhwc_f32(xg.ptr, bad.ptr, N, H, W, C, _stream()) == CNL_E_UNSUPPORTED and bad.untouched()
    RAN.add(("maxpool", "3x3 s2"))


@pytest.mark.parametrize("entry", ["f32 split", "f32 matrix cores", "fused max-pool", "uint8", "uint8 + fused max-pool"])
@pytest.mark.parametrize("shape", [(2, 37, 70), (3, 6, 10)], ids=lambda t: "N{}_{}x{}".format(*t))
def test_stem_writes_only_its_output(entry, shape):
    """The stem entries: the input through its four element strides (a 3-channel slice of NHWC pixels 7 elements apart, at element offset 2, NaN / 255
    around it), the 64-channel output packed inside guards; y_absmax: one slot per image."""
    lib = _lib.load()
    N, H, W = shape
    g = torch.Generator().manual_seed(H)
    u8 = entry.startswith("uint8")
    pool = "max-pool" in entry
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.1
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.full((lib.cnl_stem_packed_weight_floats(),), float("nan"), device="cuda")
    _lib.check(lib.cnl_stem_pack_weights_f32(wd.data_ptr(), wp.data_ptr(), _stream()))
    bd = b.cuda()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if pool:
        Ho, Wo = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    ld, off = 7, 2
    if u8:
        xu = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
        buf = torch.full((N, H, W, ld), 255, dtype=torch.uint8)
        buf[..., off:off + 3] = xu
        xd = buf.cuda()
        xptr = xd.data_ptr() + off
        mean = torch.tensor([0.485, 0.456, 0.406]) * 255
        istd = 1.0 / (torch.tensor([0.229, 0.224, 0.225]) * 255)
        xf = ((xu.float() - mean) * istd).permute(0, 3, 1, 2).contiguous()
    else:
        xg = _g((N, H, W), 3, (off, ld - 3), torch.randn(N, H, W, 3, generator=g), "x")
        xptr = xg.ptr
        xf = xg.result().permute(0, 3, 1, 2).contiguous()
    yg, ym = _g((N, Ho, Wo), 64, (0, 0)), _slots(N)
    sn, sc, sh, sw = H * W * ld, 1, W * ld, ld
    if u8:
        m3, s3 = (ctypes.c_float * 3)(*mean.tolist()), (ctypes.c_float * 3)(*istd.tolist())
        rc = lib.cnl_stem_conv7x7_u8(xptr, sn, sc, sh, sw, m3, s3, wp.data_ptr(), bd.data_ptr(), yg.ptr, ym.ptr, N, H, W, int(pool), _stream())
    elif pool:
        rc = lib.cnl_stem_conv7x7_maxpool_f32(xptr, sn, sc, sh, sw, wp.data_ptr(), bd.data_ptr(), yg.ptr, ym.ptr, N, H, W, _stream())
    else:
        algo = CNL_ALGO_F32 if entry == "f32 matrix cores" else CNL_ALGO_AUTO
        rc = lib.cnl_stem_conv7x7_f32(xptr, sn, sc, sh, sw, wp.data_ptr(), bd.data_ptr(), yg.ptr, ym.ptr, N, H, W, algo, _stream())
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    for ok, msg in (yg.verdict(), ym.verdict(_slot_only())):
        assert ok, msg
    y = yg.result()
    assert yg.unwritten() == 0 and not torch.isnan(y).any() and (u8 or xg.unchanged())
    split = entry != "f32 matrix cores"
    cls = "stem_split" if split else "stem_f32"
    pl = (lambda t: F.max_pool2d(t, 3, 2, 1)) if pool else (lambda t: t)
    z, sc64, fl = rp._conv_parts(xf.double(), w.double(), b.double(), 2, 3, CNL_RELU, None, None, split)
    ratio, where = rp._worst(rp._nchw(y), pl(F.relu(z)), pl(rp.U * sc64 + fl))
    print(f"    stem {entry}: ratio {ratio:.3f} (R_CLASS {rp.R_CLASS[cls]})")
    assert ratio <= rp.R_CLASS[cls], (ratio, where)
    if split:
        assert torch.equal(_slot_values(ym), y.abs().amax(dim=(1, 2, 3)))
    RAN.add(("stem", entry))


# ---------------------------------------------------------------------------------------------------------------------------- coverage
REQUIRED = ({("conv2d", d[0]) for d in DIRECT} | {("conv2d", "out_add, 16-byte epilogue"), ("conv2d", "out_add, scalar epilogue"), ("conv2d", "rejections")} |
            {("winograd", f"variant {v}, forced") for v in (2, 5, 6, 9, 10, 11, 13)} |
            {("winograd", f"variant {v}, default") for v in (2, 5, 6, 9, 10, 11, 13)} |
            {("winograd", "variant 9 + upsample_in, default"), ("winograd", "variant 9 + w_up, default"), ("winograd", "variant 9 + fuse_w, default"),
             ("winograd", "variant 9, own absmax pass"), ("winograd", "alignment fallback to 2 / 5 / 6"), ("winograd", "fuse_w refused on a layout variant 9 cannot take"),
             ("winograd", "Cout % 4 != 0 excluded from the row kernels")} |
            {("winograd", f"forced {v} on a layout it cannot take") for v in (6, 9, 10, 11, 13)} |
            {("fused_out_reduce", "16-byte store"), ("fused_out_reduce", "element stores"), ("up2", "fp32"), ("up2", "fp16-split")} |
            {("pointwise", f"tile shape {t}") for t in range(4)} |
            {("pointwise", f) for f in ("one source", "one source, residual", "two sources, stride2 1, residual", "two sources, stride2 2", "two sources, stride2 2, residual")} |
            {("deconv", f"K={K}") for K in (2, 3, 4)} | {("upsample2x", "mode 0"), ("upsample2x", "mode 1")} |
            {("fuse_sum", (m, t)) for m in range(4) for t in (False, True)} | {("depthwise", "3x3"), ("maxpool", "3x3 s2")} |
            {("deform_sample", f"K={K} mask={m}") for K, m in ((3, True), (3, False), (1, True))} |
            {("stem", e) for e in ("f32 split", "f32 matrix cores", "fused max-pool", "uint8", "uint8 + fused max-pool")})


def test_the_strided_launches_reach_every_entry_and_form(capsys):
    """The (entry, form) pairs that ran under a strided layout in this module (it runs after the tests above) contain the whole list: a parametrisation
    cannot quietly run nothing."""
    with capsys.disabled():
        print("\n[strided io] (entry, form) pairs exercised under strided layouts:")
        for e, f in sorted(RAN, key=str):
            print(f"    {e}: {f}")
    missing = REQUIRED - RAN
    assert not missing, "never ran under a strided layout: " + "; ".join(str(m) for m in sorted(missing, key=str))
