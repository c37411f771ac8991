"""GPU: cnl_letterbox_yuv420_u8 and letterbox_yuv420 / tile_yuv420 / detect_frames(pixel_format=...) / detect_tiled(pixel_format=...).

Every comparison is torch.equal / array_equal on BYTES: the conversion and the resize are integer arithmetic, so the canvas must equal
tests/yuv_ref.letterbox_yuv420_ref (the conversion rule, then the existing numpy letterbox rule) and the existing RGB kernels fed the
oracle's converted frames, with no tolerance to choose."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ref_cpu
import yuv_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")

# 1080p, 720p, portrait, the smallest frame, tiny and extreme-aspect frames (up- and down-scaled by both targets)
MIXED = [(1080, 1920), (720, 1280), (1280, 720), (2, 2), (16, 8), (34, 1000), (1000, 34)]
TARGETS = [(512, 512), (608, 1088)]
COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
FILL = (114, 7, 201)


def mixed_planes(seed, sizes=MIXED):
    rng = np.random.default_rng(seed)
    return [yuv_ref.random_planes(rng, h, w) for (h, w) in sizes]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, extra):
    """The array inside a wider device buffer (row stride > width), as a view."""
    buf = torch.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], 0xEE, dtype=torch.uint8, device="cuda")
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def device_frames(planes, form):
    """The host planes as device frames in one of the accepted forms."""
    out = []
    for i, (y, u, v) in enumerate(planes):
        if form == "nv12":                           # (a), NV12
            out.append(dev(yuv_ref.to_nv12(y, u, v)))
        elif form == "i420":                         # (a), I420
            out.append(dev(yuv_ref.to_i420(y, u, v)))
        elif form == "nv12_surface":                 # (a) with a pitch larger than the width: a decoder surface
            out.append(pitched(yuv_ref.to_nv12(y, u, v), 64 + 2 * i))
        elif form == "y_uv":                         # (b), each plane with its own pitch
            out.append((pitched(y, 37 + i), pitched(np.stack([u, v], axis=-1), 5 + i)))
        elif form == "y_u_v":                        # (c), pitched: U and V share a pitch
            out.append((pitched(y, 13 + i), pitched(u, 9), pitched(v, 9)))
        else:
            raise AssertionError(form)
    return out


def layout_of(form):
    return "i420" if form in ("i420", "y_u_v") else "nv12"


def build(cfg_name):
    torch.manual_seed(0)
    model = cl.build_centernet(os.path.join(CONFIGS, cfg_name))
    model.load_state_dict(ref_cpu.synth_state_dict(model.state_dict(), seed=0, calib_shape=(2, 3, 128, 128)))
    return model.cuda()


# ----------------------------------------------------------------------------- the canvas against the oracle
@pytest.mark.parametrize("form", ["nv12", "i420", "nv12_surface", "y_uv", "y_u_v"])
@pytest.mark.parametrize("height,width", TARGETS)
def test_canvas_is_bit_identical_to_the_oracle_and_to_the_rgb_kernel(height, width, form):
    planes = mixed_planes(seed=10 + len(form))
    for y, u, v in planes[:3]:
        assert y.min() == 0 and y.max() == 255 and u.min() == 0 and u.max() == 255 and v.min() == 0 and v.max() == 255
    frames = device_frames(planes, form)
    for matrix, full_range in COMBOS:
        ref, geo = yuv_ref.letterbox_yuv420_ref(planes, height, width, FILL, matrix, full_range)
        canvas, geom = cl.letterbox_yuv420(frames, height, width, layout=layout_of(form), matrix=matrix, full_range=full_range, fill=FILL)
        assert tuple(canvas.shape) == (len(planes), height, width, 3) and canvas.dtype == torch.uint8
        assert geom.frames == geo and tuple(geom.table.shape) == (len(planes), 5)
        got = canvas.cpu().numpy()
        bad = np.argwhere(got != ref)
        print(f"yuv letterbox {height}x{width} {form} {matrix} full={full_range}: {got.size} bytes compared, {len(bad)} differ")
        assert got.shape == ref.shape and len(bad) == 0, (form, matrix, full_range, bad[:5].tolist())
        # ... and to the existing RGB kernel on the oracle's converted frames
        rgb = [dev(yuv_ref.yuv420_to_rgb(y, u, v, matrix, full_range)) for (y, u, v) in planes]
        want, g2 = cl.letterbox.letterbox_uint8(rgb, height, width, fill=FILL)
        assert torch.equal(canvas, want) and g2.frames == geom.frames
    # black fill is the default
    a, _ = cl.letterbox_yuv420(frames, height, width, layout=layout_of(form))
    assert torch.equal(a, torch.from_numpy(yuv_ref.letterbox_yuv420_ref(planes, height, width, (0, 0, 0))[0]).cuda())


def test_every_saturation_branch_runs_on_the_inputs():
    """The random planes reach below 0 and above 255 in every channel before the clamp, for every coefficient set."""
    planes = mixed_planes(seed=14)
    y, u, v = (np.concatenate([p[i].reshape(-1)[:p[1].size] for p in planes]).astype(np.int64) for i in range(3))
    for matrix, full_range in COMBOS:
        y_off, cy, cvr, cvg, cug, cub = yuv_ref.coefficients(matrix, full_range)
        yy = np.maximum(y - y_off, 0) * cy + (1 << 19)
        for ch in ((yy + cvr * (v - 128)) >> 20, (yy + cvg * (v - 128) + cug * (u - 128)) >> 20, (yy + cub * (u - 128)) >> 20):
            assert ch.min() < 0 and ch.max() > 255 and ((ch > 0) & (ch < 255)).any()


def test_unletterbox_takes_the_geometry_and_a_batch_tensor_is_n_frames():
    planes = mixed_planes(seed=3)
    frames = device_frames(planes, "nv12")
    rgb = [dev(yuv_ref.yuv420_to_rgb(y, u, v)) for (y, u, v) in planes]
    _, geom = cl.letterbox_yuv420(frames, 608, 1088)
    _, want = cl.letterbox.letterbox_uint8(rgb, 608, 1088)
    boxes = torch.from_numpy(np.random.default_rng(1).uniform(-50, 1150, (len(planes), 64, 4)).astype(np.float32)).cuda()
    for clip in (True, False):
        assert torch.equal(cl.letterbox.unletterbox(boxes, geom, clip), cl.letterbox.unletterbox(boxes, want, clip))
    same = [yuv_ref.random_planes(np.random.default_rng(5 + i), 270, 480) for i in range(3)]
    stack = torch.stack([dev(yuv_ref.to_i420(*p)) for p in same])
    a, _ = cl.letterbox_yuv420(stack, 512, 512, layout="i420")
    b, _ = cl.letterbox_yuv420([dev(yuv_ref.to_i420(*p)) for p in same], 512, 512, layout="i420")
    assert torch.equal(a, b) and torch.equal(a, torch.from_numpy(yuv_ref.letterbox_yuv420_ref(same, 512, 512, (0, 0, 0))[0]).cuda())


# ----------------------------------------------------------------------------- the C ABI: every byte written once, nothing beyond
@pytest.mark.parametrize("height,width", TARGETS)
def test_c_abi_writes_every_canvas_byte_and_nothing_after_it(height, width):
    planes = mixed_planes(seed=8)
    N = len(planes)
    keep, rec = [], np.zeros((N, 9), dtype=np.int64)
    i32 = rec.view(np.int32).reshape(N, 18)
    for n, (y, u, v) in enumerate(planes):
        h, w = y.shape
        ty, tuv = dev(y), dev(np.stack([u, v], axis=-1))
        keep += [ty, tuv]
        rec[n, :3] = (ty.data_ptr(), tuv.data_ptr(), tuv.data_ptr() + 1)
        i32[n, 6:17] = (w, w, 2, 0, 0, h, w) + cl.letterbox_geometry(h, w, height, width)
    assert rec.nbytes == N * ctypes.sizeof(_lib.Yuv420Frame)
    table = torch.from_numpy(rec).cuda()
    guard = 4096
    # first pass, random planes: the canvas equals the oracle's (which holds a few genuine 0xA5 bytes) and the guard band is untouched
    buf = torch.full((N * height * width * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    coef = (ctypes.c_int32 * 6)(*cl.yuv_coefficients())
    lib = _lib.load()
    _lib.check(lib.cnl_letterbox_yuv420_u8(table.data_ptr(), buf.data_ptr(), N, height, width, coef, 0x030201,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "cnl_letterbox_yuv420_u8")
    torch.cuda.synchronize()
    got = buf[:-guard].view(N, height, width, 3).cpu().numpy()
    ref, _ = yuv_ref.letterbox_yuv420_ref(planes, height, width, (1, 2, 3))
    assert (buf[-guard:] == 0xA5).all(), "bytes after the canvas were written"
    assert np.array_equal(got, ref)
    # second pass: grey frames (Y 16..99, no chroma) convert to bytes <= 97 and the border is (1, 2, 3), so not one 0xA5 may survive
    rng = np.random.default_rng(2)
    grey = [(rng.integers(16, 100, y.shape, dtype=np.uint8), np.full(u.shape, 128, np.uint8), np.full(v.shape, 128, np.uint8)) for (y, u, v) in planes]
    for n, (y, u, v) in enumerate(grey):
        ty, tuv = dev(y), dev(np.stack([u, v], axis=-1))
        keep += [ty, tuv]
        rec[n, :3] = (ty.data_ptr(), tuv.data_ptr(), tuv.data_ptr() + 1)
    table = torch.from_numpy(rec).cuda()
    buf.fill_(0xA5)
    _lib.check(lib.cnl_letterbox_yuv420_u8(table.data_ptr(), buf.data_ptr(), N, height, width, coef, 0x030201,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "cnl_letterbox_yuv420_u8")
    torch.cuda.synchronize()
    assert not (buf[:-guard] == 0xA5).any() and (buf[-guard:] == 0xA5).all()
    assert np.array_equal(buf[:-guard].view(N, height, width, 3).cpu().numpy(), yuv_ref.letterbox_yuv420_ref(grey, height, width, (1, 2, 3))[0])


# ----------------------------------------------------------------------------- tiles
@pytest.mark.parametrize("form", ["nv12_surface", "y_u_v"])
def test_tiles_equal_tile_uint8_on_the_converted_frames(form):
    sizes = [(1080, 1920), (1000, 1500), (300, 400)]
    planes = mixed_planes(seed=40, sizes=sizes)
    frames = device_frames(planes, form)
    odd = 0
    for overlap, matrix, full_range in ((0.2, "bt601", False), (0.1, "bt709", True), (0.1, "bt601", False)):
        rgb = [dev(yuv_ref.yuv420_to_rgb(y, u, v, matrix, full_range)) for (y, u, v) in planes]
        want, wg = cl.tile_uint8(rgb, 512, 512, overlap, True, FILL)
        got, gg = cl.tile_yuv420(frames, 512, 512, overlap, True, FILL, layout=layout_of(form), matrix=matrix, full_range=full_range)
        assert gg.views == wg.views and gg.frame_first_view == wg.frame_first_view and gg.sizes == wg.sizes == sizes
        assert torch.equal(gg.merge_table, wg.merge_table) and torch.equal(gg.first_view, wg.first_view) and tuple(gg.table.shape) == (len(gg), 5)
        assert torch.equal(got, want), (overlap, matrix, np.argwhere((got != want).cpu().numpy())[:5].tolist())
        ref = yuv_ref.tile_yuv420_ref(planes, 512, 512, overlap, True, FILL, matrix, full_range)
        assert ref[3] == gg.views and np.array_equal(got.cpu().numpy(), ref[0])
        odd += sum(1 for (_, y0, x0, _, _) in gg.views if y0 % 2 or x0 % 2)
        print(f"yuv tiles {form} overlap {overlap}: {len(gg)} views, {got.numel()} bytes equal")
    assert odd > 0, "no window with an odd origin was exercised"           # overlap 0.1 of 512: a step of 461
    got, gg = cl.tile_yuv420(frames, 256, 384, 0.25, False, layout=layout_of(form))      # without the full view, another tile size
    want, wg = cl.tile_uint8([dev(yuv_ref.yuv420_to_rgb(*p)) for p in planes], 256, 384, 0.25, False)
    assert gg.views == wg.views and torch.equal(got, want)


# ----------------------------------------------------------------------------- end to end
DETECT = [(1080, 1920), (720, 1280), (1280, 720), (2, 2), (16, 8), (334, 518)]


def same_dict(a, b):
    assert set(a) == set(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("config", ["resnet34_fpn.yaml", "tracking_resnet34_fpn.yaml"])
def test_detect_frames_and_detect_tiled_equal_the_rgb_path(config):
    model = build(config)
    planes = mixed_planes(seed=21, sizes=DETECT)
    for matrix, full_range in (("bt601", False), ("bt709", True)):
        rgb = [dev(yuv_ref.yuv420_to_rgb(y, u, v, matrix, full_range)) for (y, u, v) in planes]
        want = model.detect_frames(rgb, 256, 320, fill=FILL, num_detections=50)
        got = model.detect_frames(device_frames(planes, "nv12_surface"), 256, 320, fill=FILL, num_detections=50, pixel_format="nv12", matrix=matrix,
                                  full_range=full_range)
        same_dict(got, want)
        assert ("embeddings" in got) == config.startswith("tracking")
        big = planes[:3]
        want = model.detect_tiled(rgb[:3], tile=(256, 256), overlap=0.1, batch=16, fill=FILL, score_threshold=0.0, max_detections=60)
        got = model.detect_tiled(device_frames(big, "i420"), tile=(256, 256), overlap=0.1, batch=16, fill=FILL, score_threshold=0.0,
                                 max_detections=60, pixel_format="i420", matrix=matrix, full_range=full_range)
        same_dict(got, want)
        assert int(got["count"].min()) > 0
        got = model.detect_tiled(device_frames(big, "y_u_v"), tile=(256, 256), overlap=0.1, batch=16, fill=FILL, score_threshold=0.0,
                                 max_detections=60, pixel_format="i420", matrix=matrix, full_range=full_range)
        same_dict(got, want)
    # "rgb" is the default and takes RGB frames as before
    same_dict(model.detect_frames(rgb, 256, 320, pixel_format="rgb"), model.detect_frames(rgb, 256, 320))


# ----------------------------------------------------------------------------- determinism; N = 1 and N = 33
def test_two_runs_agree_and_batches_of_1_and_33_equal_the_frames_alone():
    sizes = (MIXED * 5)[:33]
    planes = mixed_planes(seed=77, sizes=sizes)
    for form in ("nv12", "y_u_v"):
        frames = device_frames(planes, form)
        a, ga = cl.letterbox_yuv420(frames, 512, 512, layout=layout_of(form), fill=FILL)
        b, _ = cl.letterbox_yuv420(frames, 512, 512, layout=layout_of(form), fill=FILL)
        assert a.shape[0] == 33 and torch.equal(a, b)
        for i, f in enumerate(frames):
            alone, g1 = cl.letterbox_yuv420([f], 512, 512, layout=layout_of(form), fill=FILL)
            assert g1.frames == [ga.frames[i]] and torch.equal(alone[0], a[i]), (form, i, sizes[i])
        rev, _ = cl.letterbox_yuv420(frames[::-1], 512, 512, layout=layout_of(form), fill=FILL)
        assert torch.equal(rev.flip(0), a)
        t1, _ = cl.tile_yuv420(frames[:3], 512, 512, 0.1, layout=layout_of(form))
        t2, _ = cl.tile_yuv420(frames[:3], 512, 512, 0.1, layout=layout_of(form))
        assert torch.equal(t1, t2)
