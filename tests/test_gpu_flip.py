"""GPU: cnl_flip_merge_f32, cnl_mirror_append_u8 and flip_test=True on the model surface against tests/flip_ref.py.

Every comparison is an equality of fp32 bit patterns (NaN positions must match) or of bytes: the rule is one IEEE add and one multiply
by 0.5, so there is no tolerance to choose."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bench
import flip_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, flip

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")

# W = 1 and odd W; W not a multiple of 4; mirrored 4-column groups that straddle 16-byte boundaries (6, 130); more than one wave per row
SIZES = [(1, 1, 1), (1, 2, 2), (3, 5, 7), (2, 4, 6), (2, 3, 64), (2, 2, 130)]
# (C, swap_lr) of the three maps one call carries.  The box map (C = 4, swap_lr) takes the channels-last path in the channels-last
# layouts and the plane path in "nchw"; C = 80 / 64 are whole vectors per pixel, C = 5 / 1 fall to single elements per pixel
CHANNELS = {"80-box-64": ((80, False), (4, True), (64, False)), "5-box-1": ((5, False), (4, True), (1, False))}
LAYOUTS = ["nhwc", "nchw", "sliced", "separate", "mixed"]
SENTINEL = 777.0


def planted(t, N, swap_lr):
    """Special values in the logical [2N, C, H, W] tensor, as PAIRS that meet in one output element: two denormals, a denormal and a
    zero, two negative zeros, an inf and a NaN beside ordinary numbers."""
    C, H, W = t.shape[1:]
    p = flip_ref.perm(C, swap_lr)
    pairs = [(1e-45, 3e-45), (-3e-39, 0.0), (-0.0, -0.0), (float("inf"), 1.0), (float("nan"), 1.0), (2.0, float("-inf"))]
    total = N * C * H * W
    for i, (va, vb) in enumerate(pairs[:total]):
        flat = (i * 7919 + total // 3) % total if total > len(pairs) else i
        n, rest = divmod(flat, C * H * W)
        c, rest = divmod(rest, H * W)
        y, x = divmod(rest, W)
        t[n, c, y, x] = va
        t[N + n, p[c], y, W - 1 - x] = vb
    return t


def channels_last(t):
    """A logical-NCHW view of a dense NHWC copy on the GPU (what the engine returns)."""
    return t.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


def padded(t, fill=0.0):
    """[..., :C] of a dense NHWC tensor with C + 3 channels: channel stride 1, pixels 4-byte aligned only -> (logical view, whole tensor)."""
    n, c, h, w = t.shape
    big = torch.full((n, h, w, c + 3), fill, dtype=torch.float32)
    big[..., :c] = t.permute(0, 2, 3, 1)
    big = big.cuda()
    return big[..., :c].permute(0, 3, 1, 2), big


def operands(t, N, layout):
    """-> (a, b, dst, guard): the halves of t and the destination in one layout; guard() checks what must not have been written."""
    C, H, W = t.shape[1:]
    guard = lambda: True
    if layout == "nhwc":
        g = channels_last(t)
        a, b = g[:N], g[N:]
        dst = torch.full((N, H, W, C), SENTINEL, device="cuda").permute(0, 3, 1, 2)
    elif layout == "nchw":
        g = t.contiguous().cuda()
        a, b = g[:N], g[N:]
        dst = torch.full((N, C, H, W), SENTINEL, device="cuda")
    elif layout == "sliced":
        g, _ = padded(t)
        a, b = g[:N], g[N:]
        dst, big = padded(torch.full((N, C, H, W), SENTINEL), SENTINEL)
        guard = lambda: bool((big[..., C:] == SENTINEL).all())
    elif layout == "separate":
        a, b = channels_last(t[:N]), channels_last(t[N:])
        dst = torch.full((N, H, W, C), SENTINEL, device="cuda").permute(0, 3, 1, 2)
    else:                                                           # "mixed": channels-last + planes -> planes (the general strided path)
        a, b = channels_last(t[:N]), t[N:].contiguous().cuda()
        dst = torch.full((N, C, H, W), SENTINEL, device="cuda")
    return a, b, dst, guard


def merge_call(entries, N, H, W):
    """One call of cnl_flip_merge_f32: entries = [(a, b, dst, swap_lr)] of logical-NCHW tensors with any strides."""
    table = (_lib.FlipMap * len(entries))()
    for rec, (a, b, dst, swap) in zip(table, entries):
        rec.a, rec.b, rec.dst = a.data_ptr(), b.data_ptr(), dst.data_ptr()
        rec.a_sn, rec.a_sc, rec.a_sh, rec.a_sw = a.stride()
        rec.b_sn, rec.b_sc, rec.b_sh, rec.b_sw = b.stride()
        rec.d_sn, rec.d_sc, rec.d_sh, rec.d_sw = dst.stride()
        rec.C, rec.swap_lr = a.shape[1], int(swap)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().cnl_flip_merge_f32(table, len(entries), N, H, W, stream), "cnl_flip_merge_f32")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("channels", sorted(CHANNELS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_flip_merge_against_the_rule(size, channels, layout):
    N, H, W = size
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    entries, wants, guards = [], [], []
    for C, swap in CHANNELS[channels]:
        t = planted(torch.randn((2 * N, C, H, W), generator=g), N, swap)
        a, b, dst, guard = operands(t, N, layout)
        entries.append((a, b, dst, swap))
        wants.append(flip_ref.merge(t, swap))
        guards.append(guard)
    merge_call(entries, N, H, W)
    torch.cuda.synchronize()
    for (a, b, dst, swap), want, guard in zip(entries, wants, guards):
        assert flip_ref.same_bits(dst, want), (size, a.shape[1], swap, layout)
        assert guard(), (size, a.shape[1], layout, "bytes beyond the destination's channels were written")


@pytest.mark.parametrize("layout", ["nhwc", "nchw", "mixed"])
def test_flip_merge_keeps_denormals(layout):
    N, H, W = 2, 3, 10
    t = torch.randn((2 * N, 4, H, W), generator=torch.Generator().manual_seed(5)) * 1e-40
    assert bool((t.abs() < 1.1754944e-38).all())
    want = flip_ref.merge(t, True)
    assert bool((want != 0).any()) and bool((want.abs() < 1.1754944e-38).all())
    a, b, dst, _ = operands(t, N, layout)
    merge_call([(a, b, dst, True)], N, H, W)
    assert flip_ref.same_bits(dst, want)


def test_flip_merge_wrapper_returns_the_engines_layout():
    N, H, W = 2, 5, 12
    g = torch.Generator().manual_seed(9)
    outs = cl.TrackingOutput(*(channels_last(torch.randn((2 * N, C, H, W), generator=g)) for C in (3, 4, 64)))
    got = cl.flip_merge(outs, N)
    assert type(got) is cl.TrackingOutput
    want = flip_ref.merge_outputs(outs)
    for name, t in zip(got._fields, got):
        assert tuple(t.shape) == (N,) + tuple(want[name].shape[1:]) and t.permute(0, 2, 3, 1).is_contiguous(), name
        assert flip_ref.same_bits(t, want[name]), name
    # a dict of contiguous NCHW maps (reference-style callers), four maps: two calls
    d = {name: t.contiguous() for name, t in zip(outs._fields, outs)}
    d["extra"] = d["heatmap"].clone()
    got = cl.flip_merge(d, N)
    assert type(got) is dict and list(got) == list(d)
    for name in d:
        assert flip_ref.same_bits(got[name], flip_ref.merge(d[name], name == "box_2d")), name


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("size", [(1, 1, 1), (2, 3, 2), (3, 5, 67)], ids=lambda s: "x".join(map(str, s)))
def test_mirror_append_against_the_rule(size, C):
    N, H, W = size
    u8 = torch.randint(0, 256, (N, H, W, C), generator=torch.Generator().manual_seed(N + H + W + C), dtype=torch.uint8)
    got = cl.mirror_append_uint8(u8.cuda())
    assert got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(got.cpu(), flip_ref.mirror_append(u8))


# ----------------------------------------------------------------------------- the model surface
_MODELS = {}


def model_of(config):
    if config not in _MODELS:
        torch.manual_seed(0)
        _MODELS[config] = bench.synthetic_weights_(cl.build_centernet(os.path.join(CONFIGS, bench.CONFIGS[config]))).cuda()
    return _MODELS[config]


def frames_of(config):
    n, h, w = (2, 64, 96) if config == "simple" else (1, 64, 64)
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).cuda()


def as_dict(out):
    return dict(out) if isinstance(out, dict) else dict(zip(out._fields, out))


def assert_maps_equal(got, want, what):
    got = as_dict(got)
    assert list(got) == list(want), what
    for name in want:
        assert flip_ref.same_bits(got[name], want[name]), (what, name)


@pytest.mark.parametrize("config", ["simple", "tracking"])
def test_flip_test_is_the_merge_of_the_doubled_forward(config):
    model, frames = model_of(config), frames_of(config)
    doubled = torch.cat((frames, frames.flip(2)))
    assert torch.equal(cl.mirror_append_uint8(frames), doubled)
    assert_maps_equal(model.forward_uint8(frames, flip_test=True), flip_ref.merge_outputs(model.forward_uint8(doubled)), "forward_uint8")
    x = model.preprocess_uint8(frames)
    x2 = torch.cat((x, x.flip(-1)))
    got = model.forward(x, flip_test=True)
    assert type(got) is (cl.TrackingOutput if config == "tracking" else cl.DetectionOutput)
    assert_maps_equal(got, flip_ref.merge_outputs(model.forward(x2)), "forward")
    assert_maps_equal(model(x, flip_test=True), flip_ref.merge_outputs(model(x2)), "__call__")
    got = model.get_encoded_outputs(x, flip_test=True)
    assert isinstance(got, dict)
    assert_maps_equal(got, flip_ref.merge_outputs(model.get_encoded_outputs(x2)), "get_encoded_outputs (logits)")
    # the merged maps have the engine's layout: the decode takes them as it takes a plain forward's
    for t in model.forward_uint8(frames, flip_test=True):
        assert t.shape[0] == frames.shape[0] and t.permute(0, 2, 3, 1).is_contiguous()


@pytest.mark.parametrize("config", ["simple", "tracking"])
def test_flip_test_is_exactly_mirror_equivariant(config):
    """The merged maps of the mirrored frames are the mirror of the merged maps of the frames (columns reversed, box channels 0 and 2
    swapped), bit for bit: both are 0.5 * (net(frame) + mirror(net(mirrored frame))) with the operands of the one add exchanged.
    A dropped swap_lr or a column index off by one breaks it."""
    model, frames = model_of(config), frames_of(config)
    assert not torch.equal(frames, frames.flip(2))
    here = as_dict(model.forward_uint8(frames, flip_test=True))
    there = as_dict(model.forward_uint8(frames.flip(2).contiguous(), flip_test=True))
    assert_maps_equal(there, flip_ref.mirror_maps(here), "mirror equivariance")
    plain = flip_ref.mirror_maps({"box_2d": here["box_2d"]})["box_2d"]
    assert not torch.equal(plain, here["box_2d"].cpu().flip(-1)), "the box map's left and right do not differ: the test shows nothing"


def assert_dets_equal(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        assert flip_ref.same_bits(got[key], want[key]), (what, key)


@pytest.mark.parametrize("config", ["simple", "tracking"])
def test_detect_frames_flip_test_equals_the_hand_composition(config):
    model = model_of(config)
    g = torch.Generator().manual_seed(21)
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda() for (h, w) in ((40, 60), (64, 33))]
    canvas, geom = model.letterbox_uint8(frames, 64, 64)
    merged = cl.flip_merge(model.forward_uint8(cl.mirror_append_uint8(canvas)), len(frames))
    gather = model.gather_tracking2d if config == "tracking" else model.gather_detection2d
    want = gather(merged, num_detections=100, nms_kernel=3, normalize_bbox=False)
    want["bboxes"] = model.unletterbox(want["bboxes"], geom, True)
    got = model.detect_frames(frames, height=64, width=64, flip_test=True)
    assert_dets_equal(got, want, "detect_frames")
    assert not torch.equal(got["scores"], model.detect_frames(frames, height=64, width=64)["scores"])


def test_detect_tiled_flip_test_equals_the_hand_composition():
    model = model_of("simple")
    frame = torch.randint(0, 256, (100, 150, 3), generator=torch.Generator().manual_seed(31), dtype=torch.uint8).cuda()
    views, geom = model.tile_uint8([frame], 64, 64, 0.2, True, (0, 0, 0))
    V = views.shape[0]
    assert V > 3 and V % 3 != 0, V                                  # a chunk boundary inside the view list, and a short last chunk
    parts = []
    for i in range(0, V, 3):
        chunk = views[i:i + 3]
        merged = cl.flip_merge(model.forward_uint8(cl.mirror_append_uint8(chunk)), chunk.shape[0])
        parts.append(model.gather_detection2d(merged, num_detections=100, nms_kernel=3, normalize_bbox=False))
    dets = {key: torch.cat([p[key] for p in parts]) for key in parts[0]}
    m = model.merge_tiles(dets["bboxes"], dets["scores"], dets["labels"], geom, max_detections=50, score_threshold=0.0)
    want = {key: m[key] for key in ("bboxes", "labels", "scores", "count")}
    got = model.detect_tiled([frame], tile=(64, 64), batch=3, max_detections=50, score_threshold=0.0, flip_test=True)
    assert int(got["count"][0]) > 0
    assert_dets_equal(got, want, "detect_tiled")


def test_flip_test_false_is_the_call_without_the_keyword():
    model, frames = model_of("simple"), frames_of("simple")
    x = model.preprocess_uint8(frames)
    for name, arg in (("forward_uint8", frames), ("forward", x), ("get_encoded_outputs", x)):
        fn = getattr(model, name)
        a, b = as_dict(fn(arg, flip_test=False)), as_dict(fn(arg))
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), name
    fr = [frames[0], frames[1, :40, :50].contiguous()]
    a, b = model.detect_frames(fr, height=64, width=64, flip_test=False), model.detect_frames(fr, height=64, width=64)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    kw = dict(tile=(64, 64), batch=3, max_detections=20, score_threshold=0.0)
    a, b = model.detect_tiled([frames[0]], flip_test=False, **kw), model.detect_tiled([frames[0]], **kw)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
