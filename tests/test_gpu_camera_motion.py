"""GPU: CameraMotion / cnl_camera_motion_u8 (csrc/camera_motion.hip) held EQUAL to tests/camera_motion_ref.py — shift, used, vectors, sad and
status, call by call — at the smallest shapes where the kernels can go wrong: odd coarse sizes and ragged row ends, both block sizes, one block
and 256 blocks, mixed sizes with a subset of the streams, every pixel format at a pitch wider than the frame, the foreground mask, a size
change, reset(stream), two torch streams; and, through the C ABI, outputs and coarse planes inside guard bytes."""
import ctypes

import numpy as np
import pytest
import torch

import camera_motion_ref as cr
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from strided_io import GuardedBytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 32
SMALL = dict(downscale=2, grid=(3, 4), block=8, radius=4)           # shifts up to 8 pixels in steps of 2
KEYS = ("shift", "used", "vectors", "sad", "status")


@pytest.fixture(scope="module")
def canvas():
    return cr.textured(np.random.default_rng(0), 256 + 2 * MARGIN, 320 + 2 * MARGIN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(out, want, where):
    for key in KEYS:
        got = out[key].cpu().numpy()
        assert got.dtype == want[key].dtype and got.shape == want[key].shape, (where, key)
        bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        assert np.array_equal(got.view(bits), want[key].view(bits)), (where, key, got, want[key])


def both(S, **cfg):
    return cl.CameraMotion(S, **cfg), cr.CameraMotion(S, **cfg)


def view(canvas, h, w, shift):
    return cr.window(canvas, h, w, MARGIN, shift)


def test_small_mixed_frames_call_by_call(canvas):
    """96 x 128 and 70 x 90 (coarse 35 x 45: odd sizes, rows of 270 bytes that end inside a 16-pixel chunk) at d = 2, B = 8, R = 4."""
    got, want = both(2, **SMALL)
    sizes = [(96, 128), (70, 90)]
    moves = [[(0, 0), (0, 0)], [(4, -2), (-8, 8)], [(4, -2), (0, 6)], [(-2, 0), (8, -2)]]
    for t, shifts in enumerate(moves):
        frames = [view(canvas, h, w, s) for (h, w), s in zip(sizes, shifts)]
        ref = want.update(frames)
        same(got.update([dev(f) for f in frames]), ref, t)
        if t:
            assert ref["shift"].tolist() == [[a - c, b - d] for (a, b), (c, d) in zip(shifts, moves[t - 1])] and ref["used"].tolist() == [12, 12]


def test_the_default_rule_on_one_frame(canvas):
    """256 x 320 at d = 4, B = 16, R = 8, 8 x 8 blocks: 289 candidates per block, the 32 x 32 window."""
    got, want = both(1)
    for t, s in enumerate([(0, 0), (12, -8), (-20, 24), (12, -8)]):
        f = view(canvas, 256, 320, s)
        ref = want.update([f])
        same(got.update([dev(f)]), ref, t)
    assert ref["shift"][0].tolist() == [32, -32] and ref["used"][0] == 64


@pytest.mark.parametrize("grid, block", [((1, 1), 16), ((1, 1), 8), ((16, 16), 16), ((16, 1), 8), ((2, 16), 8)])
def test_one_block_and_256_blocks(canvas, grid, block):
    got, want = both(1, grid=grid, block=block, min_blocks=1)
    for t, s in enumerate([(0, 0), (-4, 28)]):
        f = view(canvas, 200, 320, s)
        ref = want.update([f])
        same(got.update([dev(f)]), ref, (grid, t))
    assert ref["shift"][0].tolist() == [-4, 28] and ref["used"][0] == grid[0] * grid[1]


@pytest.mark.parametrize("downscale, radius", [(1, 8), (2, 5), (4, 1), (8, 3)])
def test_every_downscale(canvas, downscale, radius):
    """Every d (the coarse kernel's instantiations), radii that leave the window rows off a dword boundary; 131 x 203: leftover rows and columns."""
    got, want = both(1, downscale=downscale, grid=(2, 3), block=8, radius=radius, min_blocks=1)
    for t, s in enumerate([(0, 0), (downscale, -downscale)]):
        f = view(canvas, 131 if downscale < 8 else 256, 203 if downscale < 8 else 315, s)
        ref = want.update([f])
        same(got.update([dev(f)]), ref, (downscale, t))
    assert ref["shift"][0].tolist() == [downscale, -downscale]


def test_three_streams_mixed_sizes_and_subsets(canvas):
    got, want = both(3, **SMALL)
    sizes = {0: (96, 128), 1: (71, 93), 2: (128, 160)}
    calls = [([0, 1, 2], [(0, 0)] * 3), ([2, 0], [(2, 2), (-4, 6)]), ([1], [(8, -8)]), ([1, 2, 0], [(8, -6), (0, 0), (-4, 0)])]
    for t, (streams, shifts) in enumerate(calls):
        frames = [view(canvas, *sizes[s], sh) for s, sh in zip(streams, shifts)]
        ref = want.update(frames, streams=streams)
        same(got.update([dev(f) for f in frames], streams=streams), ref, t)
    assert ref["shift"].tolist() == [[0, 2], [-2, -2], [0, -6]] and ref["status"].tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="streams"):
        got.update([dev(frames[0])], streams=[3])
    with pytest.raises(ValueError, match="one frame per stream"):
        got.update([dev(frames[0])], streams=[0, 1])


def _pitched(plane, extra):
    """A copy of `plane` ([h, w] or [h, w, C]) as a view of a wider allocation filled with 0xEE -> (view, allocation)."""
    h, w = plane.shape[:2]
    wide = torch.full((h, w + extra) + tuple(plane.shape[2:]), 0xEE, dtype=torch.uint8, device=DEV)
    wide[:, :w] = dev(plane)
    return wide[:, :w], wide


def test_every_pixel_format_at_a_wide_pitch(canvas):
    """RGB and RGBA against the restatement on the packed frame; NV12 and I420 against the restatement on the Y plane, and equal to grey RGB of
    the same plane.  Every frame is a view of a wider allocation, read in place and left as it was."""
    h, w = 96, 128
    rng = np.random.default_rng(5)
    results = {}
    for fmt in ("rgb", "rgba", "grey", "nv12", "i420"):
        got, want = both(1, **SMALL)
        for t, s in enumerate([(0, 0), (6, -4), (-2, 4)]):
            rgb = view(canvas, h, w, s)
            y = cr.luma(rgb).astype(np.uint8)
            allocs = []
            if fmt in ("rgb", "rgba", "grey"):
                packed = {"rgb": rgb, "rgba": np.concatenate([rgb, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], 2), "grey": np.stack([y] * 3, 2)}[fmt]
                frame, alloc = _pitched(packed, 5)
                allocs.append(alloc)
                ref, kw = want.update([rgb if fmt != "grey" else y]), {}
            else:
                chroma = rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)
                if fmt == "nv12":
                    frame, alloc = _pitched(np.concatenate([y, chroma.reshape(h // 2, w)]), 6)
                    allocs.append(alloc)
                else:
                    (yp, a0), (up, a1), (vp, a2) = _pitched(y, 10), _pitched(chroma[..., 0], 3), _pitched(chroma[..., 1], 3)
                    frame = (yp, up, vp)
                    allocs += [a0, a1, a2]
                ref, kw = want.update([y]), dict(pixel_format=fmt)
            before = [a.clone() for a in allocs]
            out = got.update([frame], **kw)
            torch.cuda.synchronize()
            same(out, ref, (fmt, t))
            assert all(torch.equal(a, b) for a, b in zip(allocs, before)), fmt
            results[fmt, t] = {k: out[k].cpu().numpy() for k in KEYS}
    for t in range(3):
        for fmt in ("nv12", "i420"):
            assert all(np.array_equal(results[fmt, t][k], results["grey", t][k]) for k in KEYS)
    assert results["rgb", 2]["shift"].tolist() == [[-8, 8]]
    with pytest.raises(ValueError, match="3 .RGB. or 4 .RGBA. channels"):
        cl.CameraMotion(1).update([torch.zeros((64, 64, 1), dtype=torch.uint8, device=DEV)])


def test_boxes_with_count_gating_and_a_nan_box(canvas):
    h, w = 128, 160
    got, want = both(2, **SMALL)
    first = [view(canvas, h, w, (0, 0))] * 2
    want.update(first)
    got.update([dev(f) for f in first])
    frames = [view(canvas, h, w, (4, 4)), view(canvas, h, w, (-6, 2))]
    boxes = np.zeros((2, 4, 4), np.float32)
    boxes[0] = [[20, 10, 90, 70], [np.nan, 0, 500, 500], [0, 0, np.inf, 400], [0, 0, 400, 400]]       # slot 0: count 3 leaves the frame-wide box dead
    boxes[1] = [[0, 0, 400, 400], [10, 10, 20, 20], [0, 0, 0, 0], [0, 0, 0, 0]]                         # slot 1: count 0 leaves every box dead
    count = np.array([3, 0], np.int32)
    ref = want.update(frames, boxes=boxes, count=count)
    same(got.update([dev(f) for f in frames], boxes=dev(boxes), count=dev(count)), ref, "count")
    assert ref["shift"].tolist() == [[4, 4], [-6, 2]] and 0 < ref["used"][0] < 12 and ref["used"][1] == 12
    got, want = both(2, **SMALL)                    # without count every box is live: both slots are masked entirely
    want.update(first)
    got.update([dev(f) for f in first])
    ref = want.update(frames, boxes=boxes)
    same(got.update([dev(f) for f in frames], boxes=dev(boxes)), ref, "no count")
    assert ref["used"].tolist() == [0, 0] and ref["status"].tolist() == [2, 2]


def test_a_size_change_and_reset_of_one_stream(canvas):
    got, want = both(2, **SMALL)
    script = [("update", [(96, 128), (96, 128)], [(0, 0), (0, 0)]),
              ("update", [(96, 128), (70, 90)], [(2, 2), (2, 2)]),            # stream 1 changes size: no previous frame
              ("update", [(96, 128), (70, 90)], [(4, 0), (4, 0)]),
              ("reset", 0, None),
              ("update", [(96, 128), (70, 90)], [(6, 0), (6, 0)]),            # stream 0 starts again
              ("update", [(128, 160), (96, 128)], [(6, 2), (6, 2)]),          # both grow: new planes
              ("update", [(128, 160), (96, 128)], [(0, 2), (8, 2)])]
    statuses = []
    for t, (what, a, b) in enumerate(script):
        if what == "reset":
            got.reset(a)
            want.reset(a)
            continue
        frames = [view(canvas, h, w, s) for (h, w), s in zip(a, b)]
        ref = want.update(frames)
        same(got.update([dev(f) for f in frames]), ref, t)
        statuses.append(ref["status"].tolist())
    assert statuses == [[3, 3], [0, 3], [0, 0], [3, 0], [3, 3], [0, 0]] and ref["shift"].tolist() == [[-6, 0], [2, 0]]


def test_a_side_stream_then_the_default_stream(canvas):
    """The second call runs under another stream than the first, with nothing in between: it finishes the first call's stream itself."""
    got, want = both(1)
    frames = [view(canvas, 256, 320, s) for s in [(0, 0), (8, 8), (-4, 0)]]
    d_frames = [dev(f) for f in frames]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    outs = []
    for t, f in enumerate(d_frames):
        if t == 1:
            outs.append(got.update([f]))
        else:
            with torch.cuda.stream(side):
                outs.append(got.update([f]))
    torch.cuda.synchronize()
    for t, f in enumerate(frames):
        same(outs[t], want.update([f]), t)


def test_outputs_and_coarse_planes_inside_guard_bytes(canvas):
    """cnl_camera_motion_u8 through the C ABI: every output at exactly its documented alignment and both streams' coarse planes at odd
    addresses, all inside guard bytes; the pitched frames sit inside 0xEE bytes.  Two calls (the second reads the first's planes)."""
    lib = _lib.load()
    cfg = dict(SMALL)
    d, (gy, gx) = cfg["downscale"], cfg["grid"]
    nb, sizes, L = gy * gx, [(70, 90), (96, 131)], 2
    want = cr.CameraMotion(L, **cfg)
    planes = [[GuardedBytes((h // d) * (w // d), align=1, device=DEV, name=f"plane {i}.{p}") for p in (0, 1)] for i, (h, w) in enumerate(sizes)]
    for t, shifts in enumerate([[(0, 0), (0, 0)], [(2, -8), (-6, 4)]]):
        frames = [view(canvas, h, w, s) for (h, w), s in zip(sizes, shifts)]
        pitched = [_pitched(f, 7) for f in frames]
        before = [a.clone() for _, a in pitched]
        outs = {"shift": GuardedBytes(8 * L, align=4, device=DEV, name="shift"), "used": GuardedBytes(4 * L, align=4, device=DEV, name="used"),
                "vectors": GuardedBytes(4 * nb * L, align=2, device=DEV, name="vectors"), "sad": GuardedBytes(4 * nb * L, align=4, device=DEV, name="sad"),
                "status": GuardedBytes(4 * L, align=4, device=DEV, name="status")}
        rec = np.zeros((L, 5), np.int64)
        for i, ((v, _), (h, w)) in enumerate(zip(pitched, sizes)):
            rec[i, :3] = v.data_ptr(), planes[i][t].ptr, planes[i][1 - t].ptr if t else 0
            rec[i, 3:].view(np.int32)[:3] = h, w, v.stride(0)
        table = dev(rec)
        args = _lib.CameraMotion(table.data_ptr(), None, None, *(outs[k].ptr for k in KEYS), L, 0, 3, d, gy, gx, cfg["block"], cfg["radius"], 4, 24, 4, 0)
        assert lib.cnl_camera_motion_u8(ctypes.byref(args), 7, None) == 0, _lib.last_error()
        torch.cuda.synchronize()
        ref = want.update(frames)
        dtypes = {"shift": torch.float32, "used": torch.int32, "vectors": torch.int16, "sad": torch.int32, "status": torch.int32}
        same({k: outs[k].result(dtypes[k], ref[k].shape) for k in KEYS}, ref, t)
        for g in list(outs.values()) + [p for pair in planes for p in pair]:
            ok, msg = g.verdict()
            assert ok, msg
        for i in range(L):
            assert np.array_equal(planes[i][t].result(torch.uint8).numpy(), want.prev[i].astype(np.uint8).reshape(-1)), (t, i)
            if not t:
                assert planes[i][1].untouched()
        assert all(torch.equal(a, b) for (_, a), b in zip(pitched, before))
    assert ref["shift"].tolist() == [[2, -8], [-6, 4]]


def _boom(*a, **kw):
    raise AssertionError("host synchronisation inside CameraMotion.update")


def test_update_never_synchronises_on_one_stream(canvas, monkeypatch):
    got, want = both(2, **SMALL)
    moves = [[(0, 0), (0, 0)], [(2, 2), (-4, 6)], [(0, 0), (-8, 0)], [(6, -8), (0, 0)]]
    frames = [[view(canvas, h, w, s) for (h, w), s in zip([(96, 128), (70, 90)], shifts)] for shifts in moves]
    d_frames = [[dev(f) for f in fs] for fs in frames]
    boxes = torch.tensor([[[10.0, 10.0, 60.0, 50.0]]] * 2, device=DEV)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        for owner, attr in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item"),
                            (torch.Tensor, "tolist"), (torch.Tensor, "numpy")):
            m.setattr(owner, attr, _boom)
        outs = [got.update(fs, boxes=boxes) for fs in d_frames]
        got.reset(1)
        outs.append(got.update(d_frames[0]))
    for t, fs in enumerate(frames):
        same(outs[t], want.update(fs, boxes=boxes.cpu().numpy()), t)
    want.reset(1)
    same(outs[-1], want.update(frames[0]), "after reset")
