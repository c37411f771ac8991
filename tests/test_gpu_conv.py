"""GPU: layer-level parity of the HIP conv / stem / max-pool kernels (called through the C ABI) against plain
PyTorch CPU fp32 ops — the ATen calls of the reference's forward (F.conv2d, F.relu, F.max_pool2d,
F.interpolate(nearest), add, sigmoid).  Tolerance: |d| <= 1e-4 + 1e-4*|ref| (north star: 1e-4 fp32); the
only difference is fp32 summation order (MFMA k-order vs oneDNN)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from centernet_lightning_amd import _lib
from centernet_lightning_amd._lib import (CNL_ALGO_AUTO, CNL_ALGO_F2, CNL_ALGO_F32, CNL_ALGO_FORCE, CNL_RELU, CNL_SIGMOID, CNL_UPSAMPLE_IN,
                                          CNL_UPSAMPLE_OUT_ADD, ConvParams)

pytestmark = pytest.mark.gpu
RTOL = ATOL = 1e-4


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_conv(x_nchw, w_oihw, bias, stride=1, flags=0, residual=None, ldx_extra=0, x_off=0, hints=False, algo=CNL_ALGO_AUTO, splitk=0, presplit=False,
             no_wmax=False):
    """x_nchw: CPU tensor. Returns NCHW CPU output of cnl_conv2d_nhwc_f32.  hints: hand over max |x| per image (from
    cnl_absmax_per_image_f32) and max |w|, which selects the fp16-split kernel where it applies; then returns (out, kernel, y_absmax)."""
    lib = _lib.load()
    N, Cin, H, W = x_nchw.shape
    Cout, _, KH, KW = w_oihw.shape
    ldx = Cin + ldx_extra
    xb = torch.full((N, H, W, ldx), float("nan"))          # poison the padding channels
    xb[..., x_off:x_off + Cin] = x_nchw.permute(0, 2, 3, 1)
    xd = xb.cuda()
    wd = w_oihw.permute(0, 2, 3, 1).contiguous().cuda()
    bd = bias.cuda()
    p = ConvParams()
    p.x, p.w, p.bias = xd.data_ptr() + 4 * x_off, wd.data_ptr(), bd.data_ptr()
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, H, W, Cin, Cout
    p.KH, p.KW, p.stride, p.pad = KH, KW, stride, (KH - 1) // 2
    p.ldx, p.flags, p.algo = ldx, flags, algo
    if presplit:                                               # the weights with their fp16 split appended (CNL_W_SPLIT)
        nfl = lib.cnl_conv_split_weight_floats(Cin, Cout, KH, KW)
        assert nfl == 2 * wd.numel() + 4
        wbuf = torch.full((nfl,), float("nan"), device="cuda")
        _lib.check(lib.cnl_conv_split_weights_f32(wd.data_ptr(), wbuf.data_ptr(), Cin, Cout, KH, KW, _stream()), "split weights")
        assert torch.equal(wbuf[:wd.numel()], wd.reshape(-1))
        p.w, p.flags = wbuf.data_ptr(), flags | _lib.CNL_W_SPLIT
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(lib.cnl_conv2d_out_hw(ctypes.byref(p), ctypes.byref(ho), ctypes.byref(wo)))
    oh, ow = ho.value, wo.value
    if flags & CNL_UPSAMPLE_OUT_ADD:
        oh, ow = 2 * oh, 2 * ow
    y = torch.full((N, oh, ow, Cout), float("nan"), device="cuda")
    p.y, p.ldy = y.data_ptr(), Cout
    rd = None
    if residual is not None:
        rd = residual.permute(0, 2, 3, 1).contiguous().cuda()
        p.residual, p.ldr = rd.data_ptr(), Cout
    if hints:
        xm = torch.full((N * _lib.absmax_stride(),), float("nan"), device="cuda")      # (strided: one cache line per image)
        _lib.check(lib.cnl_absmax_per_image_f32(p.x, N, H * W, Cin, ldx, xm.data_ptr(), _stream()), "absmax")
        wm = wd.abs().max().reshape(1).contiguous()
        ym = _lib.absmax_buffer(N)
        p.x_absmax, p.w_absmax, p.y_absmax = xm.data_ptr(), (None if no_wmax else wm.data_ptr()), ym.data_ptr()
    if splitk:
        p.splitk = splitk
        nbytes = lib.cnl_conv2d_splitk_scratch_bytes(ctypes.byref(p))
        assert nbytes == splitk * N * ho.value * wo.value * Cout * 4
        scratch = torch.full((nbytes // 4 + 4,), float("nan"), device="cuda")
        assert lib.cnl_conv2d_nhwc_f32(ctypes.byref(p), _stream()) == _lib.CNL_E_WORKSPACE       # scratch missing
        p.splitk_scratch, p.splitk_scratch_bytes = scratch.data_ptr(), nbytes
    _lib.check(lib.cnl_conv2d_nhwc_f32(ctypes.byref(p), _stream()), "conv")
    torch.cuda.synchronize()
    if hints:
        assert torch.equal(_lib.absmax_values(xm).cpu(), x_nchw.abs().amax(dim=(1, 2, 3)))
        return y.cpu().permute(0, 3, 1, 2), lib.cnl_conv2d_kernel(ctypes.byref(p)), _lib.absmax_values(ym).cpu()
    return y.cpu().permute(0, 3, 1, 2)


def ref_conv(x, w, b, stride=1, flags=0, residual=None):
    if flags & CNL_UPSAMPLE_IN:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, w, b, stride=stride, padding=(w.shape[-1] - 1) // 2)
    if flags & CNL_UPSAMPLE_OUT_ADD:
        y = F.interpolate(y, scale_factor=2, mode="nearest") + residual
    elif residual is not None:
        y = y + residual
    if flags & CNL_RELU:
        y = F.relu(y)
    if flags & CNL_SIGMOID:
        y = y.sigmoid()
    return y


def mk(N, Cin, H, W, Cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (1.0 / (Cin * k * k)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


CASES = [
    # N, Cin, H, W, Cout, k, stride, flags, residual
    (2, 64, 16, 16, 64, 3, 1, CNL_RELU, False),            # 256x64 tile, layer1 shape
    (2, 64, 16, 16, 128, 3, 2, CNL_RELU, False),           # stride 2
    (2, 64, 16, 16, 128, 1, 2, 0, False),                  # 1x1 stride-2 downsample
    (1, 256, 8, 8, 256, 3, 1, CNL_RELU, True),             # K = 2304, residual + relu
    (2, 512, 4, 4, 512, 3, 1, CNL_RELU, True),             # K = 4608 (layer4), 64x128 tile
    (1, 256, 16, 16, 80, 1, 1, CNL_SIGMOID, False),        # heatmap out_conv + sigmoid (N tail 80 < 128)
    (1, 256, 16, 16, 4, 1, 1, 0, False),                   # box out_conv, 256x32 tile
    (1, 64, 5, 7, 64, 3, 1, CNL_RELU, False),              # ragged M (35 rows) and odd spatial size
    (3, 32, 9, 11, 160, 3, 1, 0, False),                   # Cin = 32, Cout tail over two N tiles
    (1, 128, 8, 8, 64, 3, 1, CNL_RELU | CNL_UPSAMPLE_IN, False),   # conv on nearest-2x upsampled input
    (2, 64, 6, 6, 256, 3, 1, CNL_RELU | CNL_UPSAMPLE_IN, False),
    (1, 256, 4, 4, 128, 1, 1, CNL_UPSAMPLE_OUT_ADD, True),         # Fuse: project -> up -> + skip
    (2, 512, 2, 2, 256, 1, 1, CNL_UPSAMPLE_OUT_ADD, True),
    (2, 64, 40, 40, 256, 3, 1, CNL_RELU, False),           # > 512 tiles -> 128x128 config, many K chunks
]



@pytest.mark.parametrize("case", [(1, 512, 16, 16, 512, 3, 1, 16, True), (1, 256, 32, 32, 256, 3, 1, 9, False), (2, 256, 17, 9, 96, 3, 2, 4, True),
                                  (1, 512, 16, 16, 256, 1, 1, 4, False), (3, 128, 8, 8, 130, 3, 1, 7, True), (1, 128, 12, 12, 64, 3, 1, 64, False)],
                         ids=lambda c: "N{}c{}_{}x{}_o{}k{}s{}_split{}r{}".format(*[int(v) for v in c]))
def test_split_reduction_matches_cpu_and_unsplit(case):
    """cnl_conv_params.splitk (small grids: the reduction of an output tile split over several workgroups, partial sums added in slice
    order by splitk_reduce_kernel): the path's 1e-4 tolerance against conv2d on the CPU, fp32-grade agreement with the unsplit launch,
    bias / residual / ReLU / max |y| hand-over applied once by the reduce, deterministic; without the hints the launch runs unsplit."""
    N, Cin, H, W, Cout, K, stride, split, use_res = case
    x, w, b = mk(N, Cin, H, W, Cout, K, seed=Cin + Cout + split)
    ho, wo = (H + 2 * ((K - 1) // 2) - K) // stride + 1, (W + 2 * ((K - 1) // 2) - K) // stride + 1
    res = torch.randn(N, Cout, ho, wo, generator=torch.Generator().manual_seed(3)) if use_res else None
    want = ref_conv(x, w, b, stride=stride, flags=CNL_RELU, residual=res)
    y0, k0, m0 = run_conv(x, w, b, stride=stride, flags=CNL_RELU, residual=res, hints=True)
    y1, k1, m1 = run_conv(x, w, b, stride=stride, flags=CNL_RELU, residual=res, hints=True, splitk=split)
    y2, _, _ = run_conv(x, w, b, stride=stride, flags=CNL_RELU, residual=res, hints=True, splitk=split)
    assert k1 == 5 and k0 == (5 if K == 3 else 2)            # a small 1x1 takes the fp16-split kernel only when it is split
    torch.testing.assert_close(y1, want, rtol=RTOL, atol=ATOL)
    assert float((y1 - y0).abs().max()) <= 4e-6 * float(want.abs().max())              # fp32-grade: other summation grouping / kernel
    assert torch.equal(y1, y2)                                                          # slice order is fixed
    assert torch.equal(m1, y1.abs().amax(dim=(1, 2, 3)))
    y3 = run_conv(x, w, b, stride=stride, flags=CNL_RELU, residual=res, splitk=split)   # no hints -> fp32 matrix cores, unsplit
    torch.testing.assert_close(y3, want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}c{}_{}x{}_o{}k{}s{}f{}r{}".format(*[int(v) for v in c]))
def test_conv_matches_cpu(case):
    N, Cin, H, W, Cout, k, stride, flags, use_res = case
    x, w, b = mk(N, Cin, H, W, Cout, k, seed=Cin * 7 + Cout + H)
    ref_nores = ref_conv(x, w, b, stride, flags & ~(CNL_RELU | CNL_SIGMOID | CNL_UPSAMPLE_OUT_ADD))
    res = None
    if use_res:
        shape = list(ref_nores.shape)
        if flags & CNL_UPSAMPLE_OUT_ADD:
            shape[2] *= 2
            shape[3] *= 2
        res = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    ref = ref_conv(x, w, b, stride, flags, res)
    out = run_conv(x, w, b, stride, flags, res)
    assert out.shape == ref.shape
    assert not torch.isnan(out).any()
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL)


F16X2_CASES = [c for c in CASES if not (c[7] & (CNL_UPSAMPLE_IN | CNL_UPSAMPLE_OUT_ADD))] + [
    (3, 128, 19, 34, 256, 3, 2, CNL_RELU, False),          # 608x1088 frames: tiles span images (10 x 17 = 170 rows per image)
    (5, 64, 3, 5, 96, 1, 1, 0, True),                      # several images inside one tile
    (2, 512, 16, 16, 256, 1, 1, 0, False),                 # FPN lateral
    (1, 256, 128, 128, 80, 1, 1, CNL_SIGMOID, False),      # the 80-class heatmap conv at its real size: a 1x1 the rule sends to the split kernel
]

@pytest.mark.parametrize("case", F16X2_CASES, ids=lambda c: "N{}c{}_{}x{}_o{}k{}s{}f{}r{}".format(*[int(v) for v in c]))
def test_conv_f16x2_matches_cpu(case):
    """The same layers through the fp16-split kernel (x_absmax / w_absmax handed over): same tolerance as the fp32 matrix-core
    kernel, and the max |y| per image it reports is exactly the maximum of what it stored."""
    N, Cin, H, W, Cout, k, stride, flags, use_res = case
    algo = CNL_ALGO_AUTO
    if k == 1 and (H // stride) * (W // stride) * Cout < (1 << 20):
        x, w, b = mk(N, Cin, H, W, Cout, k, seed=1)
        assert run_conv(x, w, b, stride, flags & ~CNL_SIGMOID, hints=True)[1] == 2     # the size rule keeps small 1x1 convs on fp32 ...
        algo = CNL_ALGO_FORCE + 5                                                    # ... cover the KS = 1 template anyway
    x, w, b = mk(N, Cin, H, W, Cout, k, seed=Cin * 7 + Cout + H)
    x[N - 1] *= 37.0                                       # images of different magnitude: a row's scale is its own image's
    ref_nores = ref_conv(x, w, b, stride, flags & ~(CNL_RELU | CNL_SIGMOID))
    res = torch.randn(ref_nores.shape, generator=torch.Generator().manual_seed(5)) if use_res else None
    ref = ref_conv(x, w, b, stride, flags, res)
    out, kernel, ymax = run_conv(x, w, b, stride, flags, res, hints=True, algo=algo)
    assert kernel == 5
    assert run_conv(x, w, b, stride, flags, res, hints=True, algo=CNL_ALGO_F32)[1] == 2      # the caller can pin the fp32 matrix cores
    assert out.shape == ref.shape and not torch.isnan(out).any()
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL * max(1.0, ref.abs().max().item() / 10))
    if kernel == 5:
        assert torch.equal(ymax, out.abs().amax(dim=(1, 2, 3)))


def test_conv_f16x2_exact_on_small_integers_and_batch_invariant():
    """Integers up to 2^10 split exactly (hi = x S, lo = 0), so every product and partial sum is exact: the fp16-split kernel must
    reproduce the integer result bit for bit.  And an image's rows are scaled by its own maximum: its output is the same bits
    alone or beside images 1e5 x larger / smaller."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (2, 64, 9, 9), generator=g).float()
    w = torch.randint(-4, 5, (96, 64, 3, 3), generator=g).float()
    b = torch.randint(-4, 5, (96,), generator=g).float()
    out, kernel, _ = run_conv(x, w, b, 2, 0, hints=True)
    assert kernel == 5 and torch.equal(out, ref_conv(x, w, b, 2, 0))
    x, w, b = mk(3, 128, 10, 17, 128, 3, seed=21)
    x[0] *= 1e5
    x[2] *= 1e-5
    full, _, _ = run_conv(x, w, b, 2, CNL_RELU, hints=True)
    for n in range(3):
        alone, _, _ = run_conv(x[n:n + 1], w, b, 2, CNL_RELU, hints=True)
        assert torch.equal(alone[0], full[n]), n


def test_conv_f16x2_error_not_above_fp32_mfma():
    """Error against float64 of the fp16-split direct kernel <= 1.25 x that of the fp32 matrix-core kernel on a K = 2304 layer, also
    with channels spanning six decades and with all-tiny / all-huge tensors."""
    g = torch.Generator().manual_seed(11)
    for case in ("plain", "spread", "tiny", "huge"):
        x = torch.randn(1, 256, 32, 32, generator=g).clamp_min(0)
        if case == "spread":
            x = x * torch.pow(10.0, torch.randint(-3, 4, (1, 256, 1, 1), generator=g).float())
        elif case == "tiny":
            x = x * 1e-12
        elif case == "huge":
            x = x * 1e12
        w = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        b = torch.zeros(256)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), stride=2, padding=1)
        e32 = (run_conv(x, w, b, 2, 0).double() - ref).abs().max().item()
        out, kernel, _ = run_conv(x, w, b, 2, 0, hints=True)
        assert kernel == 5 and torch.isfinite(out).all()
        e16 = (out.double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert e16 <= 1.25 * e32 + 1e-7 * scale, (case, e16, e32, scale)
        assert e16 < 2e-5 * scale, (case, e16, scale)


@pytest.mark.parametrize("case", [(2, 64, 12, 20, 96, CNL_RELU), (1, 32, 7, 5, 160, 0), (3, 128, 9, 12, 64, CNL_RELU), (2, 64, 64, 64, 128, CNL_RELU)],
                         ids=lambda c: "N{}c{}_{}x{}_o{}f{}".format(*[int(v) for v in c]))
@pytest.mark.parametrize("hints", [False, True])
def test_conv3x3_on_upsampled_input_as_subpixel_phases(case, hints):
    """cnl_conv3x3_up2_nhwc_f32: the 3x3 conv on the nearest-2x upsampled input as four 2x2 phase convs on the low-resolution input
    with pre-summed weights (fp32 matrix cores without hints, fp16-split kernel with them) against conv2d(interpolate(x))."""
    N, Cin, H, W, Cout, flags = case
    lib = _lib.load()
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=Cin + Cout + H)
    x[N - 1] *= 29.0
    ref = ref_conv(x, w, b, 1, flags | CNL_UPSAMPLE_IN)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.full((lib.cnl_up2_weight_floats(Cin, Cout),), float("nan"), device="cuda")
    _lib.check(lib.cnl_up2_pack_weights_f32(wd.data_ptr(), wp.data_ptr(), Cin, Cout, _stream()))
    bd = b.cuda()
    y = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device="cuda")
    p = ConvParams()
    p.x, p.w, p.bias, p.y = xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr()
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, H, W, Cin, Cout
    p.KH, p.KW, p.stride, p.pad = 3, 3, 1, 1
    p.ldx, p.ldy, p.flags = Cin, Cout, flags | CNL_UPSAMPLE_IN
    if hints:
        xm = _lib.absmax_pack(x.abs().amax(dim=(1, 2, 3)).cuda())
        wm = wp.abs().max().reshape(1)
        ym = _lib.absmax_buffer(N)
        p.x_absmax, p.w_absmax, p.y_absmax = xm.data_ptr(), wm.data_ptr(), ym.data_ptr()
    split = hints
    assert lib.cnl_conv3x3_up2_kernel(ctypes.byref(p)) == (5 if split else 2)
    _lib.check(lib.cnl_conv3x3_up2_nhwc_f32(ctypes.byref(p), _stream()), "up2")
    torch.cuda.synchronize()
    out = y.cpu().permute(0, 3, 1, 2)
    assert not torch.isnan(out).any()
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL * max(1.0, ref.abs().max().item() / 10))
    if split:
        assert torch.equal(_lib.absmax_values(ym).cpu(), out.abs().amax(dim=(1, 2, 3)))
        for n in range(N):                                   # batch invariance: image n alone gives the same bits
            p.N, p.x, p.y = 1, xd[n].data_ptr(), y.data_ptr()
            p.x_absmax, p.y_absmax = xm[n * _lib.absmax_stride():].data_ptr(), ym.data_ptr()
            _lib.check(lib.cnl_conv3x3_up2_nhwc_f32(ctypes.byref(p), _stream()), "up2")
            torch.cuda.synchronize()
            assert torch.equal(y[0].cpu().permute(2, 0, 1), out[n]), n


def test_conv_reads_channel_slice_of_wider_buffer():
    """heads read their 256-channel slice out of the fused 512-channel first-block buffer (ldx > Cin, x offset)."""
    x, w, b = mk(1, 64, 8, 8, 64, 3, seed=3)
    out = run_conv(x, w, b, 1, CNL_RELU, ldx_extra=64, x_off=32)
    torch.testing.assert_close(out, ref_conv(x, w, b, 1, CNL_RELU), rtol=RTOL, atol=ATOL)


def test_conv_is_deterministic():
    x, w, b = mk(2, 128, 12, 12, 128, 3, seed=9)
    a = run_conv(x, w, b, 1, CNL_RELU)
    for _ in range(2):
        assert torch.equal(a, run_conv(x, w, b, 1, CNL_RELU))


def test_conv_exact_on_integers():
    """Small-integer operands make every product and partial sum exact in fp32: any indexing / padding / swizzle
    mistake shows up as a hard mismatch, independent of summation order (asymmetric weights catch transposes)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (2, 64, 10, 9), generator=g).float()
    w = torch.randint(-2, 3, (96, 64, 3, 3), generator=g).float()
    b = torch.randint(-5, 6, (96,), generator=g).float()
    assert torch.equal(run_conv(x, w, b, 1, 0), ref_conv(x, w, b, 1, 0))
    assert torch.equal(run_conv(x, w, b, 2, CNL_RELU), ref_conv(x, w, b, 2, CNL_RELU))


@pytest.mark.parametrize("shape,channels_last", [((2, 3, 64, 64), False), ((2, 3, 64, 64), True), ((1, 3, 96, 160), False),
                                                 ((1, 3, 70, 50), True)])
def test_stem_matches_cpu(shape, channels_last):
    lib = _lib.load()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(*shape, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, b, stride=2, padding=3))
    xd = x.cuda()
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.full((lib.cnl_stem_packed_weight_floats(),), float("nan"), device="cuda")
    _lib.check(lib.cnl_stem_pack_weights_f32(wd.data_ptr(), wp.data_ptr(), _stream()))
    bd = b.cuda()
    N, _, H, W = shape
    y = torch.full((N, ref.shape[2], ref.shape[3], 64), float("nan"), device="cuda")
    sn, sc, sh, sw = xd.stride()
    _lib.check(lib.cnl_stem_conv7x7_f32(xd.data_ptr(), sn, sc, sh, sw, wp.data_ptr(), bd.data_ptr(), y.data_ptr(), None, N, H, W, CNL_ALGO_AUTO, _stream()))
    torch.cuda.synchronize()
    torch.testing.assert_close(y.cpu().permute(0, 3, 1, 2), ref, rtol=RTOL, atol=ATOL)


def _run_stem(lib, x, w, b, channels_last=False, algo=CNL_ALGO_AUTO):
    xd = x.cuda()
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.full((lib.cnl_stem_packed_weight_floats(),), float("nan"), device="cuda")
    _lib.check(lib.cnl_stem_pack_weights_f32(wd.data_ptr(), wp.data_ptr(), _stream()))
    bd = b.cuda()
    N, _, H, W = x.shape
    y = torch.full((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), float("nan"), device="cuda")
    sn, sc, sh, sw = xd.stride()
    _lib.check(lib.cnl_stem_conv7x7_f32(xd.data_ptr(), sn, sc, sh, sw, wp.data_ptr(), bd.data_ptr(), y.data_ptr(), None, N, H, W, algo, _stream()))
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2)


def test_stem_f16x2_exact_on_integers_batch_invariant_and_pad_safe():
    """The default stem kernel forms its products on the fp16 matrix cores from scaled two-way splits (csrc/stem_f16x2.hip).
    Small integers split exactly -> bit-exact result; the scale comes from the workgroup's own patch -> an image's output is the
    same bits alone or beside images 1e5 x larger / smaller; the zero-weight pad entries of its K layout are masked -> a
    non-finite pixel only reaches the outputs whose 7x7 window contains it."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(8)
    x = torch.randint(-8, 9, (2, 3, 37, 70), generator=g).float()
    w = torch.randint(-4, 5, (64, 3, 7, 7), generator=g).float()
    b = torch.randint(-4, 5, (64,), generator=g).float()
    assert torch.equal(_run_stem(lib, x, w, b), F.relu(F.conv2d(x, w, b, stride=2, padding=3)))
    x = torch.randn(3, 3, 40, 72, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    x[0] *= 1e5
    x[2] *= 1e-5
    full = _run_stem(lib, x, w, b, channels_last=True)
    for n in range(3):
        assert torch.equal(_run_stem(lib, x[n:n + 1], w, b, channels_last=True)[0], full[n]), n
    torch.testing.assert_close(full[1], F.relu(F.conv2d(x[1:2], w, b, stride=2, padding=3))[0], rtol=RTOL, atol=ATOL)
    x = torch.rand(1, 3, 64, 64, generator=g)
    x[0, 1, 21, 30] = float("inf")
    out, ref = _run_stem(lib, x, w.abs(), b), F.relu(F.conv2d(x, w.abs(), b, stride=2, padding=3))
    fin = torch.isfinite(ref)                 # (inside the window the split gives NaN where fp32 gives inf, and fmaxf-ReLU maps NaN to 0)
    assert (~fin).sum() == 64 * 12 and torch.isfinite(out[fin]).all()
    torch.testing.assert_close(out[fin], ref[fin], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 70, 134), (3, 3, 32, 96), (1, 3, 6, 10)])
def test_stem_with_fused_maxpool_is_bit_identical_to_two_launches(shape):
    """cnl_stem_conv7x7_maxpool_f32 pools the conv tile inside the stem kernel (border cells merged across workgroups with atomic
    max): the same bits as cnl_stem_conv7x7_f32 + cnl_maxpool3x3s2_nhwc_f32, for full, ragged and tiny images and both layouts."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.1
    N, _, H, W = shape
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.empty((lib.cnl_stem_packed_weight_floats(),), device="cuda")
    _lib.check(lib.cnl_stem_pack_weights_f32(wd.data_ptr(), wp.data_ptr(), _stream()))
    bd = b.cuda()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    for cl_ in (False, True):
        xd = x.cuda().contiguous(memory_format=torch.channels_last) if cl_ else x.cuda()
        sn, sc, sh, sw = xd.stride()
        y1 = torch.empty((N, Ho, Wo, 64), device="cuda")
        y2 = torch.empty((N, Hp, Wp, 64), device="cuda")
        yf = torch.full((N, Hp, Wp, 64), float("nan"), device="cuda")
        ym1, ymf = _lib.absmax_buffer(N), _lib.absmax_buffer(N)                       # y_absmax: max |y| per image, folded in by the kernel
        _lib.check(lib.cnl_stem_conv7x7_f32(xd.data_ptr(), sn, sc, sh, sw, wp.data_ptr(), bd.data_ptr(), y1.data_ptr(), ym1.data_ptr(), N, H, W, CNL_ALGO_AUTO, _stream()))
        _lib.check(lib.cnl_maxpool3x3s2_nhwc_f32(y1.data_ptr(), y2.data_ptr(), N, Ho, Wo, 64, _stream()))
        _lib.check(lib.cnl_stem_conv7x7_maxpool_f32(xd.data_ptr(), sn, sc, sh, sw, wp.data_ptr(), bd.data_ptr(), yf.data_ptr(), ymf.data_ptr(), N, H, W, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(yf, y2), (shape, cl_)
        v1, vf = _lib.absmax_values(ym1), _lib.absmax_values(ymf)
        assert torch.equal(v1, y1.amax(dim=(1, 2, 3))) and torch.equal(vf, yf.amax(dim=(1, 2, 3))) and torch.equal(v1, vf), (shape, cl_)
        ref = F.max_pool2d(F.relu(F.conv2d(x, w, b, stride=2, padding=3)), 3, 2, 1)
        torch.testing.assert_close(yf.cpu().permute(0, 3, 1, 2), ref, rtol=RTOL, atol=ATOL)


def test_stem_f16x2_error_not_above_fp32_mfma():
    """Error against float64 of the fp16-split stem <= 1.25 x that of the fp32 matrix-core stem (algo = CNL_ALGO_F32), for [0,1)
    images, normalised images and tiny / huge inputs."""
    g = torch.Generator().manual_seed(12)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.zeros(64)
    for case, x in (("unit", torch.rand(2, 3, 96, 128, generator=g)), ("normalised", torch.randn(2, 3, 96, 128, generator=g) * 1.2),
                    ("tiny", torch.rand(1, 3, 64, 64, generator=g) * 1e-12), ("huge", torch.rand(1, 3, 64, 64, generator=g) * 1e12)):
        ref = F.relu(F.conv2d(x.double(), w.double(), stride=2, padding=3))
        e32 = (_run_stem(_lib.load(), x, w, b, algo=CNL_ALGO_F32).double() - ref).abs().max().item()
        out = _run_stem(_lib.load(), x, w, b)
        assert torch.isfinite(out).all()
        e16 = (out.double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert e16 <= 1.25 * e32 + 1e-7 * scale, (case, e16, e32, scale)
        assert e32 > 0 and e16 < 2e-5 * scale, (case, e16, e32, scale)


@pytest.mark.parametrize("shape", [(2, 64, 32, 32), (1, 64, 17, 23), (1, 8, 6, 6)])
def test_maxpool_matches_cpu_bit_exact(shape):
    lib = _lib.load()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(2))
    ref = F.max_pool2d(x, 3, 2, 1)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    N, C, H, W = shape
    y = torch.empty((N, ref.shape[2], ref.shape[3], C), device="cuda")
    _lib.check(lib.cnl_maxpool3x3s2_nhwc_f32(xd.data_ptr(), y.data_ptr(), N, H, W, C, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().permute(0, 3, 1, 2), ref)


# ----------------------------------------------------------------------------- Winograd F(2x2,3x3) path
def run_winograd(x_nchw, w_oihw, bias, flags=0, residual=None, algo=CNL_ALGO_AUTO, lib=None, want=None, ymax=False, up_rows=False):
    """`want`: assert that the dispatcher reports this kernel class (2 fp32 / 5 fp16-split).  up_rows: hand over the layer's row-pair weights
    (cnl_conv_params.w_up: the row-Winograd kernel's form behind a folded upsample)."""
    lib = lib or _lib.load()
    N, Cin, Hs, Ws = x_nchw.shape
    upf = 2 if flags & CNL_UPSAMPLE_IN else 1
    H, W = Hs * upf, Ws * upf
    Cout = w_oihw.shape[0]
    xd = x_nchw.permute(0, 2, 3, 1).contiguous().cuda()
    wd = w_oihw.permute(0, 2, 3, 1).contiguous().cuda()
    u = torch.full((lib.cnl_winograd_weight_floats(Cin, Cout),), float("nan"), device="cuda")
    _lib.check(lib.cnl_winograd_transform_weights_f32(wd.data_ptr(), u.data_ptr(), Cin, Cout, _stream()))
    bd = bias.cuda()
    y = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    p = ConvParams()
    p.x, p.w, p.bias, p.y = xd.data_ptr(), u.data_ptr(), bd.data_ptr(), y.data_ptr()
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, Hs, Ws, Cin, Cout
    p.KH = p.KW = 3
    p.stride, p.pad, p.ldx, p.ldy, p.flags, p.algo = 1, 1, Cin, Cout, flags, algo
    rd = None
    if residual is not None:
        rd = residual.permute(0, 2, 3, 1).contiguous().cuda()
        p.residual, p.ldr = rd.data_ptr(), Cout
    if ymax:                                                   # also hand the input's maxima over and collect the output's
        xm = _lib.absmax_pack(x_nchw.abs().amax(dim=(1, 2, 3)).cuda())
        ym = _lib.absmax_buffer(N)
        p.x_absmax, p.y_absmax = xm.data_ptr(), ym.data_ptr()
    if up_rows:
        wu = torch.full((lib.cnl_winograd_up_weight_floats(Cin, Cout),), float("nan"), device="cuda")
        assert wu.numel() > 0
        _lib.check(lib.cnl_winograd_transform_weights_up_f32(wd.data_ptr(), wu.data_ptr(), Cin, Cout, _stream()))
        p.w_up = wu.data_ptr()
    if want is not None:
        assert lib.cnl_conv3x3_winograd_kernel(ctypes.byref(p)) == want
    _lib.check(lib.cnl_conv3x3_winograd_f32(ctypes.byref(p), _stream()), "winograd")
    torch.cuda.synchronize()
    if ymax:
        return y.cpu().permute(0, 3, 1, 2), _lib.absmax_values(ym).cpu()
    return y.cpu().permute(0, 3, 1, 2)


WINO_CASES = [
    # N, Cin, H, W, Cout, relu, residual
    (2, 64, 16, 16, 64, True, False),
    (1, 256, 32, 32, 256, True, True),         # K = 2304, residual
    (2, 64, 128, 128, 64, True, True),         # layer1 shape (many blocks)
    (1, 512, 16, 16, 512, True, True),         # layer4
    (1, 8, 6, 10, 40, False, False),           # tiny, Cout tail (40 -> padded 64), partial 16x16 block
    (2, 24, 19, 34, 96, True, False),          # odd height (608x1088 /32 grid), ragged blocks
    (1, 128, 40, 24, 128, False, True),
    (1, 256, 19, 34, 96, True, True),          # bf16-split kernel (Cin >= 256): ragged 16x16 blocks, Cout tail (96 -> 128)
    (2, 256, 48, 16, 64, False, False),        # bf16-split kernel, one cout block, no ReLU
]


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "N{}c{}_{}x{}_o{}relu{}res{}".format(*[int(v) for v in c]))
def test_winograd_matches_cpu(case):
    N, Cin, H, W, Cout, relu, use_res = case
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=Cin + Cout + H + W)
    res = torch.randn(N, Cout, H, W, generator=torch.Generator().manual_seed(6)) if use_res else None
    flags = CNL_RELU if relu else 0
    ref = ref_conv(x, w, b, 1, flags, res)
    out = run_winograd(x, w, b, flags, res)
    assert not torch.isnan(out).any()
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL)
    # and against the direct MFMA kernel: both are fp32-rounding-level restatements of the same sum
    if Cin % 32 == 0:
        torch.testing.assert_close(out, run_conv(x, w, b, 1, flags, res), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("shape", [(2, 64, 8, 8, 128), (1, 128, 16, 24, 64), (1, 32, 5, 9, 32), (1, 256, 9, 12, 128)])
def test_winograd_upsample_in(shape):
    """conv3x3 on a nearest-2x upsampled input (simple neck stages and the heads behind it), upsample folded into the gather."""
    N, Cin, H, W, Cout = shape
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=H * W + Cout)
    flags = CNL_RELU | CNL_UPSAMPLE_IN
    out = run_winograd(x, w, b, flags)
    torch.testing.assert_close(out, ref_conv(x, w, b, 1, flags), rtol=RTOL, atol=ATOL)


def test_winograd_exact_on_small_integers():
    """With small-integer inputs and weights in multiples of 4 every Winograd intermediate (the 1/2 and 1/4 factors of G g G^T
    included) is an exact fp32 integer, so layout / index mistakes show up as hard mismatches."""
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-3, 4, (2, 16, 12, 20), generator=g).float()
    w = torch.randint(-2, 3, (48, 16, 3, 3), generator=g).float() * 4
    b = torch.randint(-5, 6, (48,), generator=g).float()
    assert torch.equal(run_winograd(x, w, b, 0), ref_conv(x, w, b, 1, 0))


def test_winograd_split_kernels_exact_on_small_integers():
    """The same exactness check on a layer that takes a split-operand kernel (Cin = 256): small integers are exact in the first
    piece (and stay so under the power-of-two scaling), so every product and partial sum is exact there too."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (1, 256, 32, 32), generator=g).float()
    w = torch.randint(-2, 3, (128, 256, 3, 3), generator=g).float() * 4
    b = torch.randint(-5, 6, (128,), generator=g).float()
    for v in (5, 6, 9, 10, 11):
        assert torch.equal(run_winograd(x, w, b, 0, algo=CNL_ALGO_FORCE + v, want=5), ref_conv(x, w, b, 1, 0)), v
    assert torch.equal(run_winograd(x, w, b, 0, algo=CNL_ALGO_F2, want=5), ref_conv(x, w, b, 1, 0))


def test_winograd_is_batch_invariant_across_magnitudes():
    """An image's output must not depend on its batch neighbours (shard == full batch) — also on the fp16-split
    kernels, whose power-of-two input scale therefore is taken per image: images of very different magnitude in one launch give
    bit for bit what each gives alone."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(3, 256, 32, 32, generator=g).clamp_min(0) * torch.tensor([1.0, 1e-3, 300.0]).view(3, 1, 1, 1)
    w = torch.randn(128, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
    b = torch.randn(128, generator=g)
    for algo, want in ((CNL_ALGO_FORCE + 9, 5), (CNL_ALGO_FORCE + 10, 5), (CNL_ALGO_FORCE + 11, 5), (CNL_ALGO_FORCE + 5, 5), (CNL_ALGO_F2, 5), (CNL_ALGO_F32, 2)):
        full = run_winograd(x, w, b, CNL_RELU, algo=algo, want=want)
        for i in range(3):
            assert torch.equal(full[i:i + 1], run_winograd(x[i:i + 1], w, b, CNL_RELU, algo=algo)), (algo, i)
        torch.testing.assert_close(full, ref_conv(x, w, b, 1, CNL_RELU), rtol=RTOL, atol=ATOL * 300)


@pytest.mark.parametrize("shape", [(5, 19, 34), (4, 38, 68), (7, 9, 20), (3, 8, 8), (2, 5, 40)], ids=lambda t: "N{}_{}x{}".format(*t))
def test_winograd6_images_side_by_side_is_bit_identical_to_one_image_at_a_time(shape):
    """winograd6_kernel<STACK>: where 16-pixel blocks pad a map's width by more than two gap columns cost, the images of a launch are laid
    side by side (W + 2 apart) and the blocks tile that virtual row — work items then span two images.  Every tile is still computed from
    its own patch, with its own image's scale: the batch gives bit for bit what each image gives alone (the plain layout), residual,
    ReLU, cout tail and the per-image max |y| hand-over included; images of very different magnitude."""
    N, H, W = shape
    g = torch.Generator().manual_seed(N * 100 + W)
    mags = torch.tensor([1.0, 1e-3, 300.0, 0.05, 7.0, 1e-6, 40.0])[:N].view(N, 1, 1, 1)
    x = torch.randn(N, 128, H, W, generator=g).clamp_min(0) * mags
    w = torch.randn(256, 128, 3, 3, generator=g) * (2.0 / (128 * 9)) ** 0.5
    b = torch.randn(256, generator=g)
    res = torch.randn(N, 256, H, W, generator=g) * mags
    full = run_winograd(x, w, b, CNL_RELU, residual=res, algo=CNL_ALGO_FORCE + 6, want=5)
    hinted, ym = run_winograd(x, w, b, CNL_RELU, residual=res, algo=CNL_ALGO_FORCE + 6, ymax=True)
    assert torch.equal(hinted, full) and torch.equal(ym, full.abs().amax(dim=(1, 2, 3)))
    for i in range(N):
        one = run_winograd(x[i:i + 1], w, b, CNL_RELU, residual=res[i:i + 1], algo=CNL_ALGO_FORCE + 6)
        assert torch.equal(full[i:i + 1], one), i
    torch.testing.assert_close(full, ref_conv(x, w, b, 1, CNL_RELU, res), rtol=RTOL, atol=ATOL * 300)


def _exp_lib():
    """The experiment build (make -C csrc experiments: the superseded Winograd variants of tools/experiments/), or None."""
    import os
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libcenternet_gfx950_exp.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def test_winograd_decompositions_are_bit_identical():
    """tools/experiments/winograd1.hip (16x16-pixel blocks) and winograd2.hip (8x16) do the same arithmetic in the same order: forced onto
    the same inputs they must agree bit for bit (experiment build only)."""
    lib = _exp_lib()
    if lib is None:
        pytest.skip("experiment build absent (make -C centernet-lightning_amd/csrc experiments)")
    g = torch.Generator().manual_seed(5)
    for (N, Cin, H, W, Cout, flags, use_res) in [(2, 64, 19, 34, 96, CNL_RELU, True), (1, 256, 38, 68, 256, CNL_RELU, False),
                                                 (1, 16, 7, 5, 20, 0, False), (2, 32, 12, 20, 64, CNL_RELU | CNL_UPSAMPLE_IN, False)]:
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (Cin * 9)) ** 0.5
        b = torch.randn(Cout, generator=g)
        up = 2 if flags & CNL_UPSAMPLE_IN else 1
        res = torch.randn(N, Cout, H * up, W * up, generator=g) if use_res else None
        outs = [run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + v, lib=lib) for v in (1, 2)]
        assert torch.equal(outs[0], outs[1]), (N, Cin, H, W, Cout)
        torch.testing.assert_close(outs[0], ref_conv(x, w, b, 1, flags, res), rtol=RTOL, atol=ATOL)


def test_winograd_split_kernels_error_not_above_fp32_mfma():
    """winograd5.hip / winograd6.hip (scaled two-way fp16 split, three cross terms, F(2x2)) form fp32 products on the 16x faster matrix
    cores and accumulate in fp32: their error against float64 must be no larger than that of the fp32 matrix-core kernel on the same
    layer (K = 2304) — also with channels spanning six decades of magnitude and with a tensor whose values are all tiny or all huge
    (the scale follows the image's maximum).  With the experiment build the superseded variants 3 (exact bf16 split) and 7 are held to the F(2x2) bar."""
    exp = _exp_lib()
    g = torch.Generator().manual_seed(11)
    for case in ("plain", "spread", "tiny", "huge"):
        x = torch.randn(1, 256, 32, 32, generator=g).clamp_min(0)
        if case == "spread":
            x = x * torch.pow(10.0, torch.randint(-3, 4, (1, 256, 1, 1), generator=g).float())
        elif case == "tiny":
            x = x * 1e-12
        elif case == "huge":
            x = x * 1e12
        w = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        b = torch.zeros(256)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
        err = {}
        for v in (2, 5, 6, 9, 10, 11) + ((3, 7) if exp is not None else ()):
            out = run_winograd(x, w, b, 0, algo=CNL_ALGO_FORCE + v, lib=exp if v in (3, 7) else None)
            assert torch.isfinite(out).all(), (case, v)
            err[v] = (out.double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        for v in err:
            if v == 2:
                continue
            assert err[v] <= 1.25 * err[2] + 1e-7 * scale, (case, v, err, scale)
        assert err[2] < 2e-5 * scale, (case, err, scale)


W9_CASES = [
    # N, Cin, H, W, Cout, flags, residual — winograd9.hip / winograd10.hip (row-Winograd): 8- / 4-row x 64-pixel x 64-cout work items
    (1, 32, 8, 64, 64, 0, False),                       # one work item, two chunks (the shortest channel loop)
    (1, 32, 8, 64, 64, CNL_RELU, True),
    (2, 64, 16, 128, 64, CNL_RELU, False),              # two blocks across, two down, layer1 channels
    (1, 256, 32, 32, 256, CNL_RELU, True),              # half-empty blocks, four cout blocks, residual
    (2, 64, 19, 34, 96, CNL_RELU, True),                # ragged rows / columns / couts (96 -> 128)
    (1, 128, 40, 24, 128, 0, True),
    (3, 32, 5, 7, 4, 0, False),                         # Cout = 4: one cout quad of one block
    (1, 64, 9, 130, 72, CNL_RELU, False),               # three blocks across, the last two pixels wide
    (2, 32, 6, 10, 64, CNL_RELU | CNL_UPSAMPLE_IN, False),
    (2, 128, 12, 36, 128, CNL_RELU | CNL_UPSAMPLE_IN, False),   # folded upsample with a long channel loop (eight chunks), three items down, two across, two cout blocks
    (3, 64, 64, 64, 64, CNL_UPSAMPLE_IN, False),        # the first head block's shape in small: 64 channels behind the upsample, 96 work items
    (1, 512, 16, 16, 512, CNL_RELU, True),              # 32 chunks
    (5, 64, 24, 72, 64, CNL_RELU, False),               # several items per workgroup never happen at this size; several images do
]


@pytest.mark.parametrize("variant", [9, 10, 11])
@pytest.mark.parametrize("case", W9_CASES, ids=lambda c: "N{}c{}_{}x{}_o{}f{}r{}".format(*[int(v) for v in c]))
def test_winograd9_matches_cpu_and_reports_absmax(case, variant):
    """winograd9.hip / winograd10.hip forced on shapes that exercise their edges: the path's 1e-4 bar against conv2d on the CPU, error against
    float64 at or below the fp32 matrix-core kernel's (+ 1e-7 of the layer maximum), max |y| per image handed over exactly; and the two
    kernels — the same arithmetic chain per accumulator on different work items — agree bit for bit."""
    N, Cin, H, W, Cout, flags, use_res = case
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=Cin + Cout + H + W)
    up = 2 if flags & CNL_UPSAMPLE_IN else 1
    res = torch.randn(N, Cout, H * up, W * up, generator=torch.Generator().manual_seed(6)) if use_res else None
    ref = ref_conv(x, w, b, 1, flags, res)
    out, ym = run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + variant, want=5, ymax=True)
    assert not torch.isnan(out).any()
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL)
    assert torch.equal(ym, out.abs().amax(dim=(1, 2, 3)))
    if variant != 9:
        assert torch.equal(out, run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 9, want=5))
    ref64 = ref_conv(x.double(), w.double(), b.double(), 1, flags, res.double() if use_res else None)
    e9 = (out.double() - ref64).abs().max().item()
    e2 = (run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 2).double() - ref64).abs().max().item()
    assert e9 <= 1.25 * e2 + 1e-7 * ref64.abs().max().item(), (e9, e2)


W13_CASES = [
    # N, Cin, H, W, Cout, flags, residual — winograd13.hip (F(4,3) along x): 4-row x 128-pixel x 64-cout work items, six transform positions on four waves
    (1, 32, 4, 128, 64, 0, False),                      # one work item, two chunks
    (1, 32, 8, 64, 64, CNL_RELU, True),                 # half-empty block row, residual
    (2, 64, 16, 128, 64, CNL_RELU, False),
    (1, 256, 32, 32, 256, CNL_RELU, True),              # four cout blocks, sixteen chunks
    (2, 64, 19, 34, 96, CNL_RELU, True),                # ragged rows / columns / couts
    (3, 32, 5, 7, 4, 0, False),                         # Cout = 4: one cout quad of one block; seven pixels: the second tile is three wide
    (1, 64, 9, 130, 72, CNL_RELU, False),               # two blocks across, the second two pixels wide
    (1, 128, 6, 256, 128, CNL_RELU, True),              # two full blocks across, 1.5 items down
    (6, 32, 6, 60, 64, CNL_RELU, True),                 # packed rows: 64-column strips, two images per block row
    (9, 64, 5, 30, 32, 0, False),                       # packed rows: 32-column strips, four images per block row (a wave's tiles span two images)
    (5, 32, 8, 68, 64, CNL_RELU, False),                # packed rows: 72-column strips — block rows start anywhere inside an image (the 38 x 68 maps of 608 x 1088 frames)
]


@pytest.mark.parametrize("case", W13_CASES, ids=lambda c: "N{}c{}_{}x{}_o{}f{}r{}".format(*[int(v) for v in c]))
def test_winograd13_f43_row_kernel(case):
    """winograd13.hip (F(4,3) along x, 108 instead of 144 matrix instructions per chunk) forced on shapes that exercise its edges: the
    path's 1e-4 bar against conv2d on the CPU; error against float64 within 6 x the fp32 matrix-core kernel's (+ 1e-7 of the layer maximum) — the larger
    tile's transforms amplify rounding: measured 2.4-4.6 x, which is why the class is opt-in (CNL_ALGO_FORCE + 13) and not what AUTO takes; max |y| per
    image handed over exactly; every image alone == inside the batch, bit for bit (one scale per image, packed rows or not); packed rows == the plain
    block grid, bit for bit; deterministic."""
    N, Cin, H, W, Cout, flags, use_res = case
    g = torch.Generator().manual_seed(Cin + Cout + H + W)
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=Cin + Cout + H + W)
    if N > 1:
        x = x * torch.pow(10.0, torch.randint(-2, 3, (N, 1, 1, 1), generator=g).float())
    res = torch.randn(N, Cout, H, W, generator=g) if use_res else None
    lib = _lib.load()
    q = ConvParams()
    q.N, q.H_in, q.W_in, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.ldx, q.ldy, q.flags, q.y, q.algo = N, H, W, Cin, Cout, 3, 3, 1, 1, Cin, Cout, flags, 1 << 20, CNL_ALGO_FORCE + 13
    assert lib.cnl_conv3x3_winograd_variant(ctypes.byref(q)) == 13
    out, ym = run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 13, want=5, ymax=True)
    assert not torch.isnan(out).any()
    ref = ref_conv(x, w, b, 1, flags, res)
    ref64 = ref_conv(x.double(), w.double(), b.double(), 1, flags, res.double() if use_res else None)
    o2 = run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 2)
    for i in range(N):                                   # per image: its own magnitude sets the tolerance
        sc = float(ref64[i].abs().max())
        assert float((out[i] - ref[i]).abs().max()) <= 1e-4 * max(sc, 1.0), i
        e13 = float((out[i].double() - ref64[i]).abs().max())
        e2 = float((o2[i].double() - ref64[i]).abs().max())
        assert e13 <= 6.0 * e2 + 1e-7 * sc, (i, e13, e2, sc)
    assert torch.equal(ym, out.abs().amax(dim=(1, 2, 3)))
    assert torch.equal(out, run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 13))
    assert torch.equal(out, run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 32 + 13))           # the plain block grid
    for i in sorted({0, N // 2, N - 1}):
        assert torch.equal(out[i:i + 1], run_winograd(x[i:i + 1], w, b, flags, res[i:i + 1] if use_res else None, algo=CNL_ALGO_FORCE + 13)), i


def test_winograd13_many_items_per_workgroup_and_fallback():
    """More work items than CUs (the next item's patches and weights are requested inside the previous item's epilogue): bit for bit what each image
    gives alone, images of very different magnitude behind each other in one workgroup.  A launch the kernel cannot take (folded upsample) falls back to
    the F(2,3) row kernel."""
    g = torch.Generator().manual_seed(23)
    N = 10
    x = torch.randn(N, 64, 64, 128, generator=g).clamp_min(0) * torch.pow(10.0, torch.randint(-3, 3, (N, 1, 1, 1), generator=g).float())
    w = torch.randn(128, 64, 3, 3, generator=g) * (2.0 / (64 * 9)) ** 0.5
    b = torch.randn(128, generator=g)
    res = torch.randn(N, 128, 64, 128, generator=g)
    full, ym = run_winograd(x, w, b, CNL_RELU, res, algo=CNL_ALGO_FORCE + 13, want=5, ymax=True)      # 10 * 16 * 1 * 2 = 320 items on 256 CUs
    torch.testing.assert_close(full, ref_conv(x, w, b, 1, CNL_RELU, res), rtol=RTOL, atol=ATOL * 100)
    for i in (0, 4, 9):
        assert torch.equal(full[i:i + 1], run_winograd(x[i:i + 1], w, b, CNL_RELU, res[i:i + 1], algo=CNL_ALGO_FORCE + 13)), i
    assert torch.equal(ym, full.abs().amax(dim=(1, 2, 3)))
    q = ConvParams()
    q.N, q.H_in, q.W_in, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.ldx, q.ldy, q.y = 2, 32, 32, 64, 64, 3, 3, 1, 1, 64, 64, 1 << 20
    q.flags, q.algo = CNL_RELU | CNL_UPSAMPLE_IN, CNL_ALGO_FORCE + 13
    assert _lib.load().cnl_conv3x3_winograd_variant(ctypes.byref(q)) == 9


@pytest.mark.parametrize("shape", [(1, 256, 4, 4, 128), (2, 512, 2, 2, 256), (3, 128, 19, 34, 64), (5, 64, 3, 5, 96), (2, 64, 5, 6, 30), (2, 128, 40, 24, 64)])
def test_fuse_epilogue_reports_absmax(shape):
    """The FPN Fuse launch (1x1 project -> nearest x2 -> + skip, CNL_UPSAMPLE_OUT_ADD; reference layers.py:160-174) folds max |y| per image into
    y_absmax, so the 3x3 output conv behind it needs no pass of its own over the fused tensor: exact, also where a tile's rows span several
    images; the output is unchanged by the report.  Cout % 4 == 0 runs on transposed accumulator tiles (16 bytes of four couts per lane), Cout = 30 on
    the scalar epilogue."""
    N, Cin, H, W, Cout = shape
    x, w, b = mk(N, Cin, H, W, Cout, 1, seed=H * W + Cout)
    g = torch.Generator().manual_seed(5)
    skip = torch.randn(N, Cout, 2 * H, 2 * W, generator=g) * torch.pow(10.0, torch.randint(-2, 3, (N, 1, 1, 1), generator=g).float())
    y0 = run_conv(x, w, b, flags=CNL_UPSAMPLE_OUT_ADD, residual=skip)
    y1, kern, ym = run_conv(x, w, b, flags=CNL_UPSAMPLE_OUT_ADD, residual=skip, hints=True)
    assert kern == 2 and torch.equal(y0, y1)
    assert torch.equal(ym, y1.abs().amax(dim=(1, 2, 3)))
    torch.testing.assert_close(y1, ref_conv(x, w, b, flags=CNL_UPSAMPLE_OUT_ADD, residual=skip), rtol=RTOL, atol=ATOL)


UP_ROWS_CASES = [
    # N, Cin, Hs, Ws, Cout, flags — stored (low-resolution) size; the conv runs on the nearest-2x upsampled map
    (2, 32, 6, 10, 64, CNL_RELU),                       # two chunks (the item's first chunk is also its last but one)
    (2, 128, 12, 36, 128, CNL_RELU),                    # eight chunks, three items down, two across (ragged), two cout blocks
    (3, 64, 64, 64, 64, 0),                             # the first head block's shape in small: 96 work items, no ReLU (signed outputs)
    (2, 64, 20, 32, 96, CNL_RELU),                      # 40 rows = five items down, couts 96 -> 128
    (5, 32, 9, 17, 64, CNL_RELU),                       # 18 x 34 logical pixels: packed rows (36-column strips), the last item's rows 16, 17 of 24
    (6, 64, 16, 16, 128, CNL_RELU),                     # the 16 -> 32-pixel neck stage of 512 x 512 frames (packed)
    (1, 64, 4, 32, 32, CNL_RELU),                       # one item, Cout = 32
]


@pytest.mark.parametrize("case", UP_ROWS_CASES, ids=lambda c: "N{}c{}_{}x{}_o{}f{}".format(*[int(v) for v in c]))
def test_row_winograd_with_row_pair_weights_behind_a_folded_upsample(case):
    """ABI v12, cnl_conv_params.w_up: behind a nearest-2x upsample (reference models/layers.py:99 + 72-77) image rows 2j and 2j + 1 are one source row, and the
    row-Winograd kernel with the layer's pre-summed row-pair weights {g0, g0 + g1, g1 + g2, g2} issues two instead of three kernel rows per output row.
    Against conv2d on the upsampled input (CPU fp32: the path's 1e-4 bar) and float64: error at or below 1.25 x the fp32 matrix core's (+ 1e-7 of the layer
    maximum), max |y| exact; within rounding of the general form (w_up = NULL); a shard equals the full batch bit for bit (also across the packed-row
    decision, which looks at N); a residual sends the launch to the general form (same bits as without w_up)."""
    N, Cin, Hs, Ws, Cout, flags = case
    flags |= CNL_UPSAMPLE_IN
    g = torch.Generator().manual_seed(Cin + Hs * Ws + Cout)
    x = torch.randn(N, Cin, Hs, Ws, generator=g) * torch.pow(10.0, torch.randint(-2, 3, (N, 1, 1, 1), generator=g).float())
    if flags & CNL_RELU:
        x = x.clamp_min(0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (Cin * 9)) ** 0.5 * torch.pow(10.0, torch.randint(-1, 2, (Cout, 1, 1, 1), generator=g).float())
    b = torch.randn(Cout, generator=g)
    out, ym = run_winograd(x, w, b, flags, algo=CNL_ALGO_FORCE + 9, want=5, ymax=True, up_rows=True)
    gen = run_winograd(x, w, b, flags, algo=CNL_ALGO_FORCE + 9, want=5)
    ref = ref_conv(x, w, b, 1, flags)
    scale = ref.abs().amax(dim=(1, 2, 3), keepdim=True)
    assert ((out - ref).abs() / scale).max().item() < 1e-4
    assert torch.equal(ym, out.abs().amax(dim=(1, 2, 3)))
    ref64 = ref_conv(x.double(), w.double(), b.double(), 1, flags)
    sc64 = ref64.abs().amax(dim=(1, 2, 3), keepdim=True)
    e_up = ((out.double() - ref64).abs() / sc64).max().item()
    e_gen = ((gen.double() - ref64).abs() / sc64).max().item()
    e_f32 = ((run_winograd(x, w, b, flags, algo=CNL_ALGO_FORCE + 2).double() - ref64).abs() / sc64).max().item()
    print(f"\n[row-pair weights] error / image max: {e_up:.3e} (general form {e_gen:.3e}, fp32 matrix cores {e_f32:.3e})")
    assert e_up <= 1.25 * e_f32 + 1e-7, (e_up, e_f32)
    assert ((out - gen).abs() / scale).max().item() < 2e-6
    # batch invariance: every image alone, and the first two together
    for n in range(min(N, 2)):
        assert torch.equal(run_winograd(x[n:n + 1], w, b, flags, algo=CNL_ALGO_FORCE + 9, up_rows=True)[0], out[n])
    if N > 2:
        assert torch.equal(run_winograd(x[:2], w, b, flags, algo=CNL_ALGO_FORCE + 9, up_rows=True), out[:2])
    # with a residual the general form runs: the same bits with and without w_up
    res = torch.randn(N, Cout, 2 * Hs, 2 * Ws, generator=g)
    assert torch.equal(run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 9, up_rows=True), run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 9))


PACKED_CASES = [
    # N, Cin, H, W, Cout, flags, residual — widths that 64-pixel block rows pad: the launch's images side by side in one virtual row, W + 2 columns each
    (3, 32, 19, 34, 64, CNL_RELU, True),                # layer4 of a 608 x 1088 frame: 3 strips of 36 columns in 2 block rows (plain grid: 3)
    (5, 64, 38, 68, 96, CNL_RELU, True),                # layer3: 5 x 70 columns in 6 block rows (10), couts 96 -> 128
    (4, 32, 10, 136, 64, 0, False),                     # layer2's width: 9 block rows (12)
    (3, 32, 9, 272, 64, CNL_RELU, False),               # layer1 / head width: 13 block rows (15)
    (7, 32, 5, 14, 4, 0, False),                        # the narrowest strip (16 columns: a group of 8 tiles spans two images), Cout = 4
    (9, 32, 6, 20, 64, CNL_RELU, True),                 # 22-column strips: block rows start anywhere inside an image
    (33, 32, 4, 62, 64, CNL_RELU, False),               # 64-column strips: every block row is exactly one image + its padding columns
    (5, 32, 9, 17, 64, CNL_RELU | CNL_UPSAMPLE_IN, False),     # behind a folded nearest-2x upsample: 18 x 34 logical pixels from 9 x 17 stored ones
    (6, 64, 16, 16, 128, CNL_RELU | CNL_UPSAMPLE_IN, True),    # the 16 -> 32-pixel neck stage of 512 x 512 frames (34-column strips)
]


@pytest.mark.parametrize("variant", [9, 10, 11])
@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: "N{}c{}_{}x{}_o{}f{}r{}".format(*[int(v) for v in c]))
def test_winograd_packed_rows_are_bit_identical_to_the_plain_grid(case, variant):
    """Packed rows of the row-Winograd kernels (cnl_wino_packed_stride, winograd9.hip): images laid side by side in one virtual row so that maps
    34 / 68 / 136 / 272 pixels wide (608 x 1088 frames, reference datasets/utils.py:29-33) fill the 64-pixel block rows.  Every output keeps its
    chain of additions and its image's scale: bit-identical to the same kernel on the plain grid (FORCE + 32 + v), with images of very
    different magnitude side by side in one block row; max |y| per image exact although a wave's tiles span two images; 1e-4 against the CPU."""
    N, Cin, H, W, Cout, flags, use_res = case
    g = torch.Generator().manual_seed(Cin + Cout + H + W)
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=Cin + Cout + H + W)
    x = x * torch.pow(10.0, torch.randint(-3, 3, (N, 1, 1, 1), generator=g).float())
    up = 2 if flags & CNL_UPSAMPLE_IN else 1
    res = torch.randn(N, Cout, H * up, W * up, generator=g) if use_res else None
    packed, ym = run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + variant, want=5, ymax=True)
    plain, ym0 = run_winograd(x, w, b, flags, res, algo=CNL_ALGO_FORCE + 32 + variant, want=5, ymax=True)
    assert not torch.isnan(packed).any()
    assert torch.equal(packed, plain)
    assert torch.equal(ym, packed.abs().amax(dim=(1, 2, 3))) and torch.equal(ym0, ym)
    ref = ref_conv(x, w, b, 1, flags, res)
    for i in range(N):                                   # per image: its own magnitude sets the tolerance
        sc = float(ref[i].abs().max())
        assert float((packed[i] - ref[i]).abs().max()) <= 1e-4 * max(sc, 1.0), i
    # the default plan takes these shapes into the row-Winograd class too (packed), whatever the batch: same bits for a shard
    q = ConvParams()
    q.N, q.H_in, q.W_in, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.ldx, q.ldy, q.flags, q.y = N, H, W, Cin, Cout, 3, 3, 1, 1, Cin, Cout, flags, 1 << 20
    if H * W >= 19 * 34:                                 # (the tiny maps of this list stay where they were: not the row-Winograd class)
        assert _lib.load().cnl_conv3x3_winograd_variant(ctypes.byref(q)) in (9, 10, 11)
        auto = run_winograd(x, w, b, flags, res)
        one = run_winograd(x[:1], w, b, flags, res[:1] if use_res else None)
        assert torch.equal(auto, packed) and torch.equal(one, packed[:1])


@pytest.mark.parametrize("variant", [9, 10, 11])
def test_winograd9_many_items_per_workgroup_is_bit_identical_to_one_image_at_a_time(variant):
    """More work items than CUs (the chunk stream then runs on from one item into the next: patches, weights and the first V rows of
    item i + 1 are fetched inside the last two chunks of item i): the batch must give bit for bit what each image gives alone, with
    images of very different magnitude side by side (the scale changes between consecutive items of a workgroup)."""
    g = torch.Generator().manual_seed(21)
    N = 12
    x = torch.randn(N, 64, 64, 128, generator=g).clamp_min(0) * torch.pow(10.0, torch.randint(-3, 3, (N, 1, 1, 1), generator=g).float())
    w = torch.randn(128, 64, 3, 3, generator=g) * (2.0 / (64 * 9)) ** 0.5
    b = torch.randn(128, generator=g)
    res = torch.randn(N, 128, 64, 128, generator=g)
    full, ym = run_winograd(x, w, b, CNL_RELU, res, algo=CNL_ALGO_FORCE + variant, want=5, ymax=True)      # 9: 12 * 8 * 2 * 2 = 384 items on 256 CUs; 10: 768 on 512 workgroups
    torch.testing.assert_close(full, ref_conv(x, w, b, 1, CNL_RELU, res), rtol=RTOL, atol=ATOL * 100)
    for i in (0, 3, 7, 11):
        assert torch.equal(full[i:i + 1], run_winograd(x[i:i + 1], w, b, CNL_RELU, res[i:i + 1], algo=CNL_ALGO_FORCE + variant)), i
    assert torch.equal(ym, full.abs().amax(dim=(1, 2, 3)))


@pytest.mark.parametrize("shape", [(2, 64, 32, 32, 128, 3, 2, CNL_RELU, False), (1, 256, 128, 128, 80, 1, 1, _lib.CNL_SIGMOID, False),
                                   (2, 128, 16, 16, 256, 3, 2, CNL_RELU, False), (1, 64, 24, 40, 96, 3, 1, 0, True), (2, 96, 9, 11, 40, 3, 2, 0, False)],
                         ids=lambda c: "N{}c{}_{}x{}_o{}k{}s{}f{}r{}".format(*[int(v) for v in c]))
def test_presplit_weights_give_the_same_bits(shape):
    """CNL_W_SPLIT (weights with their fp16 split appended by cnl_conv_split_weights_f32): the fp16-split direct kernel reads the pieces
    instead of splitting every chunk's weights again — bit for bit the same output and max |y|, with or without w_absmax; a launch that
    stays on the fp32 matrix cores (no hints) ignores the tail; the reduction-split form (fp32 weights) still works beside the flag."""
    N, Cin, H, W, Cout, K, stride, flags, res = shape
    g = torch.Generator().manual_seed(41)
    x = torch.randn(N, Cin, H, W, generator=g).clamp_min(0)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (2.0 / (Cin * K * K)) ** 0.5 * torch.pow(10.0, torch.rand(Cout, 1, 1, 1, generator=g) * 2 - 1)
    b = torch.randn(Cout, generator=g)
    ho, wo = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
    r = torch.randn(N, Cout, ho, wo, generator=g) if res else None
    algo = CNL_ALGO_FORCE + 5 if K == 1 and ho * wo * Cout < (1 << 20) else CNL_ALGO_AUTO
    base, k0, ym0 = run_conv(x, w, b, stride, flags, r, hints=True, algo=algo)
    assert k0 == 5
    for no_wmax in (False, True):
        out, k1, ym1 = run_conv(x, w, b, stride, flags, r, hints=True, algo=algo, presplit=True, no_wmax=no_wmax)
        assert k1 == 5 and torch.equal(out, base) and torch.equal(ym1, ym0), no_wmax
    assert torch.equal(run_conv(x, w, b, stride, flags, r, presplit=True), run_conv(x, w, b, stride, flags, r))       # fp32 kernel: tail ignored
    if K == 3:
        sk, ks, _ = run_conv(x, w, b, stride, flags, r, hints=True, algo=algo, presplit=True, splitk=3)
        sk0, _, _ = run_conv(x, w, b, stride, flags, r, hints=True, algo=algo, splitk=3)
        assert torch.equal(sk, sk0)
    lib = _lib.load()
    assert lib.cnl_conv_split_weight_floats(48, 64, 3, 3) == 0 and lib.cnl_conv_split_weight_floats(64, 64, 3, 1) == 0 and lib.cnl_conv_split_weight_floats(64, 64, 5, 5) == 0


@pytest.mark.parametrize("variant", [9, 10, 11])
def test_winograd9_images_side_by_side_do_not_see_each_other(variant):
    """Narrow maps (W = 32): two images share a block row.  An image's first / last Winograd tile must read the convolution's zero
    padding, not the neighbour's edge pixels — also when those are Inf / NaN (a 0 multiplier would turn them into NaN): every image of
    the batch is bit for bit what it gives alone, and the non-finite image keeps its non-finite outputs to itself."""
    g = torch.Generator().manual_seed(23)
    N = 5                                                                  # (odd: the last block row holds one image and an empty half)
    x = torch.randn(N, 64, 32, 32, generator=g).clamp_min(0)
    x[1, :, :, 0] = float("inf")                                           # left edge of image 1 touches image 0's right edge
    x[1, 3, 5, 31] = float("nan")                                          # (image 1 is the right half of its block row: nothing beside this edge)
    x[2, :, 7, 31] = float("inf")                                          # right edge of image 2 touches image 3's left edge
    w = torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (64 * 9)) ** 0.5
    b = torch.randn(64, generator=g)
    full = run_winograd(x, w, b, CNL_RELU, algo=CNL_ALGO_FORCE + variant, want=5)
    for i in (0, 3, 4):
        assert torch.isfinite(full[i]).all(), i
    for i in range(N):
        alone = run_winograd(x[i:i + 1], w, b, CNL_RELU, algo=CNL_ALGO_FORCE + variant)
        assert torch.equal(full[i:i + 1].isnan(), alone.isnan()), i
        assert torch.equal(torch.nan_to_num(full[i:i + 1], nan=-1.0), torch.nan_to_num(alone, nan=-1.0)), i


def test_split_kernels_on_trained_checkpoint_like_weights():
    """weights as a trained checkpoint with BatchNorm folded has them — per-output-channel scales over four decades
    (10^U(-3, 1)), 5 % dead channels (all-zero filters), inputs in the range of a normalised image (negative values) — must not cost the
    fp16-split kernels accuracy: error against float64 PER OUTPUT CHANNEL, relative to that channel's largest output, at or below
    1.25x the fp32 matrix-core kernel's.  (winograd5/6 scale the weights per tensor: a channel 10^-3 of the largest keeps 22 - 10 bits
    in the first piece, the second piece restores them; winograd9 scales per output channel.)"""
    g = torch.Generator().manual_seed(31)
    Cin, Cout = 256, 256
    x = torch.randn(1, Cin, 32, 64, generator=g) * 1.2 - 0.3
    scale = torch.pow(10.0, torch.rand(Cout, generator=g) * 4 - 3)
    scale[torch.randperm(Cout, generator=g)[:Cout // 20]] = 0.0
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5 * scale.view(-1, 1, 1, 1)
    b = torch.randn(Cout, generator=g) * scale
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1)
    cmax = ref.abs().amax(dim=(0, 2, 3))
    live = cmax > 0
    err = {}
    for v in (2, 5, 6, 9, 10, 11):
        out = run_winograd(x, w, b, 0, algo=CNL_ALGO_FORCE + v)
        assert torch.isfinite(out).all(), v
        d = out.double() - ref
        e = d.abs().amax(dim=(0, 2, 3))
        assert float(e[~live].max()) == 0.0 if (~live).any() else True, v          # dead channels give exact zeros
        err[v] = (e[live] / cmax[live], d.pow(2).mean(dim=(0, 2, 3)).sqrt()[live] / cmax[live])
    for v in (5, 6, 9, 10, 11):
        # per channel: rms error within 1.25x the fp32 matrix core's; the MAXIMUM over a channel's 2048 outputs is a noisy statistic -> 2x
        worst_rms = float((err[v][1] / (1.25 * err[2][1] + 2e-8)).max())
        worst_max = float((err[v][0] / (2.0 * err[2][0] + 1e-7)).max())
        assert worst_rms <= 1.0 and worst_max <= 1.0, (v, worst_rms, worst_max, float(err[v][0].max()), float(err[2][0].max()))
        assert float(err[v][0].max()) <= 1.25 * float(err[2][0].max()) + 1e-7, (v, float(err[v][0].max()), float(err[2][0].max()))


def test_winograd_dispatch_is_a_function_of_shape_and_algo_only():
    """cnl_conv3x3_winograd_kernel: the kernel CLASS (the arithmetic) follows the layer shape and the caller's algo — never the batch size,
    never the environment.  (The F(4x4) class of ABI <= 9 is gone: algo 3 is rejected.)"""
    lib = _lib.load()

    def kind(N, Cin, H, W, Cout, algo):
        p = ConvParams()
        p.N, p.H_in, p.W_in, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.ldx, p.ldy, p.flags, p.algo = N, H, W, Cin, Cout, 3, 3, 1, 1, Cin, Cout, 0, algo
        return lib.cnl_conv3x3_winograd_kernel(ctypes.byref(p))

    def variant(N, Cin, H, W, Cout, algo):
        p = ConvParams()
        p.N, p.H_in, p.W_in, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.ldx, p.ldy, p.flags, p.algo = N, H, W, Cin, Cout, 3, 3, 1, 1, Cin, Cout, 0, algo
        p.y = 1 << 20                                                   # (the row-Winograd kernels ask for a 16-byte aligned output)
        return lib.cnl_conv3x3_winograd_variant(ctypes.byref(p))

    for N in (1, 7, 32):
        assert kind(N, 256, 128, 128, 256, CNL_ALGO_AUTO) == 5          # head blocks
        assert kind(N, 256, 152, 272, 256, CNL_ALGO_AUTO) == 5          # ... of 608 x 1088 frames
        assert kind(N, 256, 128, 128, 256, CNL_ALGO_F2) == 5
        assert kind(N, 256, 128, 128, 256, CNL_ALGO_F32) == 2
        assert kind(N, 256, 32, 32, 256, CNL_ALGO_AUTO) == 5            # layer3
        assert kind(N, 128, 64, 64, 128, CNL_ALGO_AUTO) == 5            # layer2
        assert kind(N, 64, 128, 128, 64, CNL_ALGO_AUTO) == 5            # layer1: row-Winograd on the fp16 matrix cores (round 3)
        assert kind(N, 64, 16, 16, 64, CNL_ALGO_AUTO) == 2              # short channel loop on a map its 64-pixel blocks would pad 4x: fp32 matrix cores
        assert kind(N, 64, 128, 128, 64, CNL_ALGO_F32) == 2
        assert kind(N, 24, 128, 128, 64, CNL_ALGO_AUTO) == 2            # Cin % 16 != 0
        # the kernel behind the class (cnl_conv3x3_winograd_variant): round 4's half-height row-Winograd items on 16-pixel-wide maps with long
        # channel loops, and wherever a row-Winograd kernel applies under the latency class — which the CALLER chooses, never the batch size
        # (within the row-Winograd class the work-item shape follows the grid size: at most 128 of winograd9's items -> its bit-identical
        # 4-row x 32-cout form, variant 11 — the only place the batch size is looked at, and it cannot change a result)
        assert variant(N, 256, 128, 128, 256, CNL_ALGO_AUTO) == (11 if N == 1 else 9)
        assert variant(N, 256, 32, 32, 256, CNL_ALGO_AUTO) == (9 if N == 32 else 11)
        assert variant(N, 512, 16, 16, 512, CNL_ALGO_AUTO) == 10 and variant(N, 512, 16, 16, 256, CNL_ALGO_AUTO) == 11
        # the 19 x 34 / 38 x 68 maps of 608 x 1088 frames: the row-Winograd class since round 5 (packed rows), on the half-height items where 8-row
        # items would pad 19 rows to 24 (rounds 1-4: the 2-D kernels, variant 6)
        assert variant(N, 512, 19, 34, 512, CNL_ALGO_AUTO) == (10 if N == 32 else 11)
        assert variant(N, 256, 38, 68, 256, CNL_ALGO_AUTO) == (11 if N == 1 else 9)
        for shp in ((256, 128, 128, 256), (256, 32, 32, 256), (128, 64, 64, 128), (64, 128, 128, 64), (512, 16, 16, 512)):
            assert variant(N, *shp, _lib.CNL_ALGO_LATENCY) == 11, shp
        assert variant(N, 24, 128, 128, 64, _lib.CNL_ALGO_LATENCY) == 2


def _local_error(out, ref64, mask):
    """(max |out - ref| over the masked outputs) / (max |ref| over the same outputs): error relative to the LOCAL magnitude."""
    d = (out.double() - ref64).abs()[mask].max().item()
    return d / ref64.abs()[mask].max().item()


@pytest.mark.parametrize("factor", [1e3, 1e4, 1e6])
@pytest.mark.parametrize("kernel", ["winograd9", "winograd10", "winograd13", "winograd5", "conv_f16x2", "stem"])
def test_split_arithmetic_with_an_outlier_inside_one_image(kernel, factor, capsys):
    """VERDICT r4 #5.  The fp16-split kernels scale an image's activations by ONE power of two taken from the image's maximum (the stem: from
    its workgroup's patch), so a value far below that maximum loses the low piece of its split to fp16 subnormals: with the maximum at
    2^13-2^14 after scaling, a value 2^-n below it keeps min(22, 38 - n) significant bits (the fp16 subnormal ulp is 2^-24).  Here ONE
    activation of the image is `factor` x the largest of the others, and the outputs whose receptive field does NOT contain it are compared
    with float64 RELATIVE TO THEIR OWN maximum, beside the fp32 matrix-core class on the same input.  Guaranteed (asserted): up to a ratio
    of 1e4 between an image's maximum and the magnitudes that matter locally the error stays at the fp32 matrix core's level (measured
    0.5-1.0 x its error; asserted <= 2 x); at 1e6 it is 2-6e-5 of the local maximum (20-130 x fp32's), still inside the path's 1e-4 bar;
    beyond that use KernelOptions(algo="f32") — the fp32 matrix cores, no split operands (include/centernet_gfx950.h)."""
    g = torch.Generator().manual_seed(int(factor) % 1000 + len(kernel))
    lib = _lib.load()
    if kernel == "stem":
        H, W = 96, 160
        x = torch.randn(1, 3, H, W, generator=g)
        w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
        b = torch.zeros(64)
        oy, ox = 37, 91
        x[0, 1, oy, ox] = factor * x.abs().max()
        ref = F.relu(F.conv2d(x.double(), w.double(), stride=2, padding=3))
        mask = torch.ones_like(ref, dtype=torch.bool)
        # the stem scales per WORKGROUP PATCH (16 x 32 conv outputs): every output of the tile that holds the outlier shares its scale — those
        # are the "local" outputs here; outputs whose 7 x 7 window contains the outlier are excluded
        ty, tx = (oy // 2) // 16 * 16, (ox // 2) // 32 * 32
        mask[:] = False
        mask[:, :, ty:ty + 16, tx:tx + 32] = True
        mask[:, :, max(0, (oy - 3 + 1) // 2):(oy + 3) // 2 + 1, max(0, (ox - 3 + 1) // 2):(ox + 3) // 2 + 1] = False
        mask &= ref > 0
        e16 = _local_error(_run_stem(lib, x, w, b), ref, mask)
        e32 = _local_error(_run_stem(lib, x, w, b, algo=CNL_ALGO_F32), ref, mask)
    else:
        N, Cin, H, W, Cout = 1, 64, 24, 64, 64
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (Cin * 9)) ** 0.5
        b = torch.zeros(Cout)
        oy, ox = 9, 30
        x[0, 5, oy, ox] = factor * x.abs().max()
        stride = 2 if kernel == "conv_f16x2" else 1
        ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)
        mask = torch.ones_like(ref, dtype=torch.bool)
        if stride == 1:
            mask[:, :, oy - 1:oy + 2, ox - 1:ox + 2] = False
        else:
            mask[:, :, (oy - 1 + 1) // 2:(oy + 1) // 2 + 1, (ox - 1 + 1) // 2:(ox + 1) // 2 + 1] = False
        if kernel == "conv_f16x2":
            out, kern, _ = run_conv(x, w, b, stride=2, hints=True)
            assert kern == 5
            e16 = _local_error(out, ref, mask)
            e32 = _local_error(run_conv(x, w, b, stride=2), ref, mask)
        else:
            v = {"winograd9": 9, "winograd10": 10, "winograd5": 5, "winograd13": 13}[kernel]
            out = run_winograd(x, w, b, algo=CNL_ALGO_FORCE + v, want=5)
            if kernel == "winograd13":
                # F(4,3): a pixel enters ALL transform positions of its four-pixel tile(s), also those of outputs whose 3 x 3 window does not contain it — it
                # cancels there exactly in exact arithmetic and to 2^-22 of ITS magnitude in the split arithmetic (F(2,3) has no such position: every input
                # of a tile is in the window of every output it reaches).  The outputs of the outlier's tiles are therefore measured separately: their error
                # grows with the outlier (another reason why the class is opt-in), everything outside them behaves like the other kernels.
                tile = mask.clone()
                mask[:, :, oy - 1:oy + 2, max(0, ox - 5):ox + 6] = False
                tile &= ~mask
                leak = _local_error(out, ref, tile)
                with capsys.disabled():
                    print(f"\n[outlier x{factor:g}] winograd13, outputs of the outlier's tiles outside its 3 x 3 window: error / local max = {leak:.3e} = {leak / factor:.2e} x the factor")
                assert leak <= 4e-7 * factor
            e16 = _local_error(out, ref, mask)
            e32 = _local_error(run_winograd(x, w, b, algo=CNL_ALGO_FORCE + 2), ref, mask)
    with capsys.disabled():
        print(f"\n[outlier x{factor:g}] {kernel}: error / local max = {e16:.3e} (fp32 matrix cores: {e32:.3e}, ratio {e16 / e32:.2f})")
    assert e32 < 2e-6
    if factor <= 1e4:      # (winograd13, the opt-in F(4,3) class: its larger transforms sit at 2.4-4.6 x the fp32 matrix core's error with or without an outlier — the admission gate of VERDICT r5 #1)
        assert e16 <= (6.0 if kernel == "winograd13" else 2.0) * e32 + 1e-7, (e16, e32)
    assert e16 <= 1e-4, (e16, e32)


def test_row_winograd_runs_a_tensor_beyond_4_gib_in_groups_of_images():
    """A C-ABI caller's launch whose tensors cross the kernels' 32-bit buffer offsets — the first blocks of the three heads of the tracking
    model fused along Cout on 34 frames of 608 x 1088: 34 x 152 x 272 x 768 floats = 4.32 GB > 4 GiB.  The row-Winograd launchers run it as
    equal groups of images (cnl_wino_images_per_launch): bit-identical to each image alone, max |y| per image exact, nothing outside written —
    and a head block READING a 256-channel slice of that tensor (pixel stride 768) takes the same route."""
    lib = _lib.load()
    N, Cin, H, W, Cout = 34, 64, 152, 272, 768
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, H, W, Cin, device="cuda", generator=g).clamp_min(0) * torch.pow(10.0, torch.randint(-2, 3, (N, 1, 1, 1), device="cuda", generator=g).float())
    w = torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, device="cuda", generator=g)
    u = torch.empty((lib.cnl_winograd_weight_floats(Cin, Cout),), device="cuda")
    _lib.check(lib.cnl_winograd_transform_weights_f32(w.data_ptr(), u.data_ptr(), Cin, Cout, _stream()))
    y = torch.full((N * H * W * Cout + 1024,), float("nan"), device="cuda")
    assert N * H * W * Cout * 4 > 1 << 32

    def launch(x_, y_, n, cin, cout, ldx, ldy, u_, b_, xm, ym):
        p = ConvParams()
        p.x, p.w, p.bias, p.y = x_, u_.data_ptr(), b_.data_ptr(), y_
        p.N, p.H_in, p.W_in, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad = n, H, W, cin, cout, 3, 3, 1, 1
        p.ldx, p.ldy, p.flags, p.algo = ldx, ldy, CNL_RELU, CNL_ALGO_AUTO
        p.x_absmax, p.y_absmax = xm, ym
        assert lib.cnl_conv3x3_winograd_variant(ctypes.byref(p)) in (9, 10, 11)
        _lib.check(lib.cnl_conv3x3_winograd_f32(ctypes.byref(p), _stream()), "winograd")

    ams = _lib.absmax_stride()
    xm = _lib.absmax_pack(x.abs().amax(dim=(1, 2, 3)))
    ym = _lib.absmax_buffer(N)
    launch(x.data_ptr(), y.data_ptr(), N, Cin, Cout, Cin, Cout, u, b, xm.data_ptr(), ym.data_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(y[N * H * W * Cout:]).all()
    yv = y[:N * H * W * Cout].view(N, H, W, Cout)
    one = torch.empty((H, W, Cout), device="cuda")
    ym1 = _lib.absmax_buffer(1)
    for i in (0, 16, 17, 33):                                 # both sides of the group boundary
        ym1.zero_()
        launch(x[i].data_ptr(), one.data_ptr(), 1, Cin, Cout, Cin, Cout, u, b, xm.data_ptr() + 4 * ams * i, ym1.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(yv[i], one), i
        assert float(_lib.absmax_values(ym)[i]) == float(one.max()) == float(_lib.absmax_values(ym1)[0]), i
    # a head block reading channels [256, 512) of the wide tensor
    w2 = torch.randn(256, 3, 3, 256, device="cuda", generator=g) * (2.0 / (256 * 9)) ** 0.5
    b2 = torch.zeros(256, device="cuda")
    u2 = torch.empty((lib.cnl_winograd_weight_floats(256, 256),), device="cuda")
    _lib.check(lib.cnl_winograd_transform_weights_f32(w2.data_ptr(), u2.data_ptr(), 256, 256, _stream()))
    z = torch.empty((N, H, W, 256), device="cuda")
    zm = _lib.absmax_buffer(N)
    launch(y.data_ptr() + 4 * 256, z.data_ptr(), N, 256, 256, Cout, 256, u2, b2, ym.data_ptr(), zm.data_ptr())
    z1 = torch.empty((H, W, 256), device="cuda")
    for i in (3, 33):
        xi = yv[i, :, :, 256:512].contiguous()
        ym1.zero_()
        launch(xi.data_ptr(), z1.data_ptr(), 1, 256, 256, 256, 256, u2, b2, ym.data_ptr() + 4 * ams * i, ym1.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(z[i], z1), i


@pytest.mark.parametrize("case", [(2, 64, 16, 64, 256, 4, False), (3, 32, 19, 34, 96, 2, True), (1, 256, 8, 128, 256, 1, True), (5, 32, 6, 20, 64, 3, False)],
                         ids=lambda c: "N{}c{}_{}x{}_o{}c2_{}sig{}".format(*[int(v) for v in c]))
def test_small_out_conv_folded_into_the_row_winograd_epilogue(case):
    """cnl_conv_params.fuse_w / fuse_part (ABI v11): the 1x1 out_conv of at most 4 channels behind a head's last 3x3 block (reference
    models/meta.py:24-30) leaves per-32-channel partial sums in the block's epilogue and cnl_fused_out_reduce_f32 adds them in order: the
    block's own output is unchanged bit for bit; the folded conv is within fp32 rounding of a 1x1 conv of that output and within the path's
    1e-4 of the CPU; deterministic; an image alone gives the same bits as inside a batch (packed rows included: widths 34 and 20)."""
    lib = _lib.load()
    N, Cin, H, W, Cout, C2, sig = case
    x, w, b = mk(N, Cin, H, W, Cout, 3, seed=Cin + Cout + H)
    g = torch.Generator().manual_seed(3)
    x = x * torch.pow(10.0, torch.randint(-2, 3, (N, 1, 1, 1), generator=g).float())
    w2 = torch.randn(C2, Cout, 1, 1, generator=g) * 0.05
    b2 = torch.randn(C2, generator=g)
    plain = run_winograd(x, w, b, CNL_RELU, algo=CNL_ALGO_FORCE + 9, want=5)

    def folded(xs):
        n = xs.shape[0]
        xd = xs.permute(0, 2, 3, 1).contiguous().cuda()
        wd = w.permute(0, 2, 3, 1).contiguous().cuda()
        u = torch.empty((lib.cnl_winograd_weight_floats(Cin, Cout),), device="cuda")
        _lib.check(lib.cnl_winograd_transform_weights_f32(wd.data_ptr(), u.data_ptr(), Cin, Cout, _stream()))
        bd, w2d, b2d = b.cuda(), w2.reshape(C2, Cout).contiguous().cuda(), b2.cuda()
        CoutP = (Cout + 63) // 64 * 64
        fw = torch.full((CoutP, 4), float("nan"), device="cuda")
        _lib.check(lib.cnl_fused_out_pack_weights_f32(w2d.data_ptr(), fw.data_ptr(), Cout, C2, _stream()))
        assert torch.equal(fw[:Cout, :C2].cpu(), w2.reshape(C2, Cout).t()) and float(fw[Cout:].abs().sum()) == 0 and float(fw[:, C2:].abs().sum()) == 0
        nb = CoutP // 32
        part = torch.full((nb, n * H * W, 4), float("nan"), device="cuda")
        y = torch.full((n, H, W, Cout), float("nan"), device="cuda")
        out = torch.full((n, H, W, C2), float("nan"), device="cuda")
        p = ConvParams()
        p.x, p.w, p.bias, p.y = xd.data_ptr(), u.data_ptr(), bd.data_ptr(), y.data_ptr()
        p.N, p.H_in, p.W_in, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad = n, H, W, Cin, Cout, 3, 3, 1, 1
        p.ldx, p.ldy, p.flags, p.algo = Cin, Cout, CNL_RELU, CNL_ALGO_AUTO
        p.fuse_w, p.fuse_part = fw.data_ptr(), part.data_ptr()
        assert lib.cnl_conv3x3_winograd_variant(ctypes.byref(p)) == 9          # whatever the grid size
        _lib.check(lib.cnl_conv3x3_winograd_f32(ctypes.byref(p), _stream()), "winograd + folded 1x1")
        _lib.check(lib.cnl_fused_out_reduce_f32(part.data_ptr(), nb, n * H * W, C2, b2d.data_ptr(), out.data_ptr(), C2, CNL_SIGMOID if sig else 0, _stream()),
                   "reduce")
        torch.cuda.synchronize()
        return y.cpu().permute(0, 3, 1, 2), out.cpu().permute(0, 3, 1, 2)

    y, out = folded(x)
    assert torch.equal(y, plain)
    want = F.conv2d(y, w2, b2)
    want = want.sigmoid() if sig else want
    scale = max(1.0, float(want.abs().max()))
    assert float((out - want).abs().max()) <= 4e-6 * scale                    # another summation order of the same fp32 products
    ref = F.conv2d(ref_conv(x, w, b, 1, CNL_RELU), w2, b2)
    ref = ref.sigmoid() if sig else ref
    for i in range(N):
        assert float((out[i] - ref[i]).abs().max()) <= 1e-4 * max(1.0, float(ref[i].abs().max())), i
    y2, out2 = folded(x)
    assert torch.equal(out, out2)
    y1, out1 = folded(x[N - 1:])
    assert torch.equal(out1[0], out[N - 1]) and torch.equal(y1[0], y[N - 1])
    # a residual / a launch that is not the row-Winograd class cannot fold
    p = ConvParams()
    p.N, p.H_in, p.W_in, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.ldx, p.ldy, p.algo = 1, 8, 8, 24, 64, 3, 3, 1, 1, 24, 64, CNL_ALGO_AUTO
    p.x = p.w = p.bias = p.y = p.fuse_w = p.fuse_part = 1 << 20
    assert lib.cnl_conv3x3_winograd_f32(ctypes.byref(p), _stream()) == _lib.CNL_E_UNSUPPORTED


def test_a_conv_with_its_own_absmax_pass_reports_max_y_into_a_slot_of_its_own():
    """Regression (tests/test_gpu_plan_replay.py): a 3x3 direct conv whose input has no reporting producer gets an explicit cnl_absmax_per_image_f32
    pass into slot s (its x_absmax); when that conv is in turn the producer of a fp16-split consumer, its y_absmax must be ANOTHER slot — sharing s
    folded max |y| into the max |x| already there, and the consumer scaled its input by up to max |x| / max |y| (here layer4's first conv at 96 x 128:
    a slot of 451 for a maximum of 285).  Every reported slot must equal max |y| of its producer's output, image by image."""
    import os
    import centernet_lightning_amd as cl
    import recipes
    import ref_cpu
    torch.manual_seed(0)
    model = cl.build_centernet(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs",
                                            "resnet34_simple.yaml"))
    model.load_state_dict(ref_cpu.synth_state_dict(model.state_dict(), seed=1, calib_shape=(2, 3, 128, 128)))
    model.set_kernel_options(reuse_buffers=False)
    model = model.cuda()
    x = recipes.images(4321, (2, 3, 96, 128)).cuda()
    model.get_encoded_outputs(x)
    torch.cuda.synchronize()
    plan = next(iter(model._engine.plans.values()))
    both = [L for L in plan.launches if isinstance(L.args, ConvParams) and L.args.x_absmax and L.args.y_absmax]
    passed = {L.args[5] for L in plan.launches if L.fn is _lib.load().cnl_absmax_per_image_f32}
    assert any(L.args.x_absmax in passed for L in both)                  # the shape of the defect is present in this plan
    n = 0
    for L in plan.launches:
        if isinstance(L.args, ConvParams) and L.args.y_absmax:
            assert L.args.y_absmax != L.args.x_absmax, L.what
            y = plan.tensor(L.keep[1])
            off = (L.args.y_absmax - plan.absmax.data_ptr()) // 4
            got = plan.absmax.view(-1)[off::_lib.absmax_stride()][:plan.N].cpu()
            assert torch.equal(got, y.abs().reshape(plan.N, -1).amax(dim=1).cpu()), L.what
            n += 1
    assert n >= 10
