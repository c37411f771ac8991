"""CPU: camera-motion compensation without a device — tests/camera_motion_ref.py (the numpy restatement of cnl_camera_motion_u8's rule) on
planted shifts, a moving foreground, flat and too-small frames, the tie order and the lower median; the shake scene's two conditions on the
reference tracker; the C-ABI entries (declared, exported, bound, argument validation) and the refusals of `camera_motion=`."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import camera_motion_ref as cr
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cnl_camera_motion_u8", "cnl_track_shift_f64")
H, W, MARGIN = 256, 320, 32


@pytest.fixture(scope="module")
def canvas():
    return cr.textured(np.random.default_rng(0), H + 2 * MARGIN, W + 2 * MARGIN)


def _pair(cm, canvas, shift, **kw):
    cm.reset()
    cm.update([cr.window(canvas, H, W, MARGIN, (0, 0))])
    return cm.update([cr.window(canvas, H, W, MARGIN, shift)], **kw)


# ----------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("shift", [(0, 0), (12, -8), (-32, 32), (20, 4), (32, -32), (-4, 0)])
def test_planted_shifts_are_recovered_exactly(canvas, shift):
    """Multiples of d = 4 within +-R * d = 32: the true shift has SAD 0 in every block, and all 64 blocks vote for it."""
    out = _pair(cr.CameraMotion(1), canvas, shift)
    assert out["shift"].dtype == np.float32 and out["shift"][0].tolist() == list(shift)
    assert out["used"][0] == 64 and out["status"][0] == 0 and not out["sad"].any()
    assert (out["vectors"][0] == (shift[0] // 4, shift[1] // 4)).all()


def test_first_frame_and_size_change_report_no_previous_frame(canvas):
    cm = cr.CameraMotion(1)
    first = cm.update([cr.window(canvas, H, W, MARGIN, (0, 0))])
    assert first["status"][0] == 1 | 2 and first["used"][0] == 0 and not first["shift"].any() and (first["sad"] == -1).all()
    other = cm.update([cr.window(canvas, H - 16, W, MARGIN, (4, 4))])
    assert other["status"][0] == 1 | 2 and not other["shift"].any()
    again = cm.update([cr.window(canvas, H - 16, W, MARGIN, (8, 4))])
    assert again["status"][0] == 0 and again["shift"][0].tolist() == [4, 0]


@pytest.mark.parametrize("shift", [(12, -8), (-16, 16)])
def test_moving_foreground_with_and_without_boxes(canvas, shift):
    """A textured 150 x 110 rectangle moves by (8, 8) whatever the camera does (d = 2: shifts up to 16).  Without boxes the blocks inside it
    vote for its motion and the median still returns the background's shift; with its box as the mask exactly the blocks whose centre lies
    in it abstain."""
    PW, PH, d = 150, 110, 2
    patch = cr.textured(np.random.default_rng(7), PH, PW)
    frames, boxes = [], []
    for (bg, x, y) in (((0, 0), 90, 70), (shift, 98, 78)):
        f = cr.window(canvas, H, W, MARGIN, bg).copy()
        f[y:y + PH, x:x + PW] = patch
        frames.append(f)
        boxes.append([[x, y, x + PW, y + PH], [np.nan, 0, 500, 500], [0, 0, 400, 400]])
    boxes = np.asarray(boxes, np.float32)[:, None]                  # [2 calls, L = 1, k = 3, 4]
    x1, y1, x2, y2 = boxes[1, 0, 0]
    inside = sum(x1 <= (x0 + 8) * d < x2 and y1 <= (y0 + 8) * d < y2 for y0 in cr.block_starts(H // d, 8, 8, 16) for x0 in cr.block_starts(W // d, 8, 8, 16))
    assert inside == 16
    for masked in (False, True):
        cm = cr.CameraMotion(1, downscale=d)
        kw = dict(boxes=boxes[1], count=np.array([2], np.int32)) if masked else {}                 # count 2: the frame-wide third box is dead
        cm.update(frames[:1])
        out = cm.update(frames[1:], **kw)
        assert out["shift"][0].tolist() == list(shift) and out["status"][0] == 0
        own = int(((out["vectors"][0] == (4, 4)).all(1) & (out["sad"][0] >= 0)).sum())              # blocks that follow the rectangle
        assert (own, out["used"][0]) == ((0, 64 - inside) if masked else (inside, 64))
    # every live box is read: with count 3 the frame-wide box masks every block; the NaN box alone masks nothing
    cm = cr.CameraMotion(1, downscale=d)
    cm.update(frames[:1])
    out = cm.update(frames[1:], boxes=boxes[1], count=np.array([3], np.int32))
    assert out["used"][0] == 0 and out["status"][0] == 2 and not out["shift"].any()
    cm.reset()
    cm.update(frames[:1])
    out = cm.update(frames[1:], boxes=boxes[1][:, 1:2])
    assert out["used"][0] == 64


def test_flat_frame_has_no_votes():
    flat = np.full((H, W, 3), 90, np.uint8)
    cm = cr.CameraMotion(1)
    cm.update([flat])
    out = cm.update([flat])
    assert out["used"][0] == 0 and out["status"][0] == 2 and not out["shift"].any() and (out["sad"] == -1).all()


def test_frame_too_small_for_the_grid(canvas):
    cm = cr.CameraMotion(1)                                         # needs 2R + B = 32 coarse pixels: 128 frame pixels
    small = cr.window(canvas, 124, W, MARGIN, (0, 0))
    cm.update([small])
    out = cm.update([small])
    assert out["status"][0] == 4 | 2 and out["used"][0] == 0 and not out["shift"].any()
    edge = cr.window(canvas, 128, 131, MARGIN, (0, 0))              # exactly 32 x 32 coarse pixels: one position for every block
    cm.reset()
    cm.update([edge])
    out = cm.update([edge])
    assert out["status"][0] == 0 and out["used"][0] == 64 and not out["shift"].any()


def test_tie_order_on_a_frame_periodic_in_x():
    """Period 8 in x at d = 1: a true shift of 4 matches at sx = -4 and sx = 4 with SAD 0 and |sx| equal: the key's last terms take -4; at a true
    shift of 0, sx = -8, 0, 8 all match and the smallest |sy| + |sx| wins."""
    rng = np.random.default_rng(2)
    tile = rng.integers(0, 256, (96, 8), dtype=np.uint8)
    plane = np.tile(tile, (1, 14))                                  # a luma plane, 96 x 112
    cm = cr.CameraMotion(1, downscale=1, grid=(3, 3), block=8, radius=8, min_blocks=1)
    cm.update([plane])
    same = cm.update([plane])
    assert (same["vectors"][0] == (0, 0)).all() and same["used"][0] == 9
    moved = cm.update([np.roll(plane, 4, axis=1)])
    assert (moved["vectors"][0] == (-4, 0)).all() and moved["shift"][0].tolist() == [-4, 0] and not moved["sad"].any()


def test_lower_median_of_an_even_number_of_votes(canvas):
    """The top half moves by (8, 16), the bottom half by (24, -8): four votes, two each.  Index (4 - 1) // 2 = 1 of the sorted values per axis:
    the smaller one, independently per axis — a shift no block voted for."""
    a = cr.window(canvas, H, W, MARGIN, (0, 0))
    b = np.concatenate([cr.window(canvas, H, W, MARGIN, (8, 16))[:H // 2], cr.window(canvas, H, W, MARGIN, (24, -8))[H // 2:]])
    cm = cr.CameraMotion(1, grid=(2, 2), min_blocks=2)
    cm.update([a])
    out = cm.update([b])
    assert out["vectors"][0].tolist() == [[2, 4], [2, 4], [6, -2], [6, -2]] and out["used"][0] == 4
    assert out["shift"][0].tolist() == [8, -8]


def test_streams_are_independent(canvas):
    cm = cr.CameraMotion(3, downscale=2, grid=(3, 4), block=8, radius=4)
    a, b = cr.window(canvas, 96, 128, MARGIN, (0, 0)), cr.window(canvas, 70, 90, MARGIN, (0, 0))
    cm.update([a, b], streams=[2, 0])
    out = cm.update([cr.window(canvas, 70, 90, MARGIN, (-6, 2)), cr.window(canvas, 96, 128, MARGIN, (4, -8))], streams=[0, 2])
    assert out["shift"].tolist() == [[-6, 2], [4, -8]] and out["status"].tolist() == [0, 0]
    assert cm.update([a], streams=[1])["status"][0] == 3


# ----------------------------------------------------------------------------------------------------------------------- the scene
def _true_shifts():
    offs = cr.offsets()
    return [(0, 0)] + [(offs[f][0] - offs[f - 1][0], offs[f][1] - offs[f - 1][1]) for f in range(1, cr.FRAMES)]


def test_the_scene_needs_the_compensation_and_the_compensation_suffices():
    dets, _, _ = cr.shake_scene()
    objects = range(5)
    assert max(abs(dx) for dx, _ in cr.JUMP.values()) > cr.SIZE[0]
    # compensated with the true shifts: one id per object, every object matched in every frame, no track ever INACTIVE
    ids, states = cr.run_scene(dets, _true_shifts())
    assert all({i[o] for i in ids if o in i} == {o} for o in objects)
    assert all(len(ids[f]) == 5 for f in range(1, cr.FRAMES))
    assert not any(st is th.TrackState.INACTIVE for frame in states for _, st in frame)
    assert len(states[-1]) == 5
    # uncompensated, motion_gate=True: the jump leaves every pair outside the gate and without overlap
    ids, states = cr.run_scene(dets, None)
    switched = [o for o in objects if len({i[o] for i in ids if o in i}) > 1]
    lost = [f for f in range(1, cr.FRAMES) if len(ids[f]) < 5]
    assert switched and lost and min(lost) == min(cr.JUMP)


def test_the_estimator_recovers_the_scenes_shifts_from_rendered_frames():
    dets, _, _ = cr.shake_scene()
    canvas = cr.textured(np.random.default_rng(1), cr.H + 2 * cr.MARGIN, cr.W + 2 * cr.MARGIN)
    cm = cr.CameraMotion(1, **cr.ESTIMATOR)
    want = _true_shifts()
    for f in range(cr.FRAMES):
        masked = f % 2 == 1                                             # with and without the detections as the foreground mask
        out = cm.update([cr.render(canvas, dets, f)], boxes=dets[f][0][None] if masked else None)
        assert out["status"][0] == (3 if f == 0 else 0)
        assert out["shift"][0].tolist() == list(want[f]), f


# ----------------------------------------------------------------------------------------------------------------------- the C ABI, the options
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.cnl_version() == _lib.ABI_VERSION == 13
    assert ctypes.sizeof(_lib.MotionFrame) == 40 and ctypes.sizeof(_lib.CameraMotion) == 112
    assert "CameraMotion" in cl.__all__ and callable(cl.CameraMotion)
    assert th.STATUS_BAD_SHIFT == 1 << 17 and th.STATUS_BAD_SHIFT != th.STATUS_OVERFLOW
    makefile = open(os.path.join(ROOT, "centernet-lightning_amd", "csrc", "Makefile")).read()
    assert "camera_motion.hip" in makefile


def _args(**kw):
    a = _lib.CameraMotion()
    for name in ("frames", "shift", "used", "vectors", "sad", "status"):
        setattr(a, name, 0x1000)
    a.L, a.k, a.step, a.downscale, a.gy, a.gx, a.block, a.radius, a.min_texture, a.max_sad, a.min_blocks = 1, 0, 3, 4, 8, 8, 16, 8, 4, 24, 4
    for name, v in kw.items():
        setattr(a, name, v)
    return a


@pytest.mark.parametrize("bad", [dict(frames=None), dict(status=None), dict(L=0), dict(L=70000), dict(k=-1), dict(step=2), dict(downscale=3),
                                 dict(downscale=16), dict(block=12), dict(radius=0), dict(radius=9), dict(gy=0), dict(gx=17), dict(min_texture=256),
                                 dict(max_sad=-1), dict(min_blocks=0), dict(boxes=0x1000), dict(count=0x1000), dict(shift=0x1002),
                                 dict(vectors=0x1001), dict(frames=0x1004), dict(boxes=0x1002, k=3)])
def test_the_estimator_entry_refuses_bad_arguments_without_a_device(bad):
    lib = _lib.load()
    rc = lib.cnl_camera_motion_u8(ctypes.byref(_args(**bad)), 7, None)
    assert rc == (_lib.CNL_E_UNSUPPORTED if bad.get("L", 0) > 65535 else _lib.CNL_E_BAD_ARG), _lib.last_error()
    assert "cnl_camera_motion_u8" in _lib.last_error()


def test_the_entries_refuse_null_and_bad_stages_without_a_device():
    lib = _lib.load()
    assert lib.cnl_camera_motion_u8(None, 7, None) == _lib.CNL_E_BAD_ARG
    for stages in (0, 8, -1):
        assert lib.cnl_camera_motion_u8(ctypes.byref(_args()), stages, None) == _lib.CNL_E_BAD_ARG
    ok = [0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 4, 2, 16, 0]
    for i, v in ((0, None), (1, None), (3, None), (4, None), (5, None), (6, None), (0, 0x1002), (1, 0x1004), (2, 0x1004), (7, 0), (7, 5000), (8, 0), (8, 5),
                 (9, 0), (9, 5000)):
        args = list(ok)
        args[i] = v
        assert lib.cnl_track_shift_f64(*args, None) == _lib.CNL_E_BAD_ARG, (i, v)
        assert "cnl_track_shift_f64" in _lib.last_error()


@pytest.mark.parametrize("kw", [dict(downscale=3), dict(downscale=0), dict(downscale=True), dict(block=12), dict(block=32), dict(radius=0), dict(radius=9),
                                dict(radius=2.5), dict(grid=(0, 4)), dict(grid=(4, 17)), dict(grid=8), dict(grid=(2, 2, 2)), dict(min_blocks=0),
                                dict(min_texture=-1), dict(max_sad=256), dict(num_streams=0)])
def test_the_constructor_refuses_bad_options(kw):
    with pytest.raises(ValueError):
        cl.CameraMotion(**{"num_streams": 2, **kw})


def test_update_checks_what_the_host_can_check():
    cm = cl.CameraMotion(2)
    frame = torch.zeros((128, 160, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP devices only"):      # no CPU fallback
        cm.update([frame, frame])
    with pytest.raises(ValueError, match="pixel_format"):
        cm.update([frame, frame], pixel_format="bgr")
    with pytest.raises(ValueError, match="streams"):
        cm.reset(stream=2)


def _dets(L, k=4, E=8):
    return torch.zeros((L, k, 4)), torch.zeros((L, k), dtype=torch.int64), torch.zeros((L, k)), torch.zeros((L, k, E))


def test_camera_motion_is_refused_where_the_boxes_live_on_the_host():
    shift = torch.zeros((2, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tracker = cl.Tracker()
        host = cl.TrackerBank(2)
        host_kalman = cl.TrackerBank(2, use_kalman=True, kalman="host")
    for call in (lambda: tracker.update(*(t[0] for t in _dets(1)), camera_motion=shift[0:1]),
                 lambda: tracker.step_batch(torch.zeros((1, 3, 32, 32)), camera_motion=shift[0:1]),
                 lambda: host.update_batch(*_dets(2), camera_motion=shift),
                 lambda: host.step_batch(torch.zeros((2, 3, 32, 32)), camera_motion=shift),
                 lambda: host_kalman.update_batch(*_dets(2), camera_motion=shift)):
        with pytest.raises(ValueError, match=r"camera_motion.*lifecycle='device'.*required"):
            call()
    with pytest.raises(ValueError, match="kalman='host'"):
        host_kalman.update_batch(*_dets(2), camera_motion=shift)


@pytest.mark.parametrize("shift", [torch.zeros((3, 2)), torch.zeros((2, 4)), torch.zeros(2), torch.zeros((2, 2), dtype=torch.float64),
                                   np.zeros((2, 2), np.float32), [[0.0, 0.0], [0.0, 0.0]]])
def test_a_wrong_shift_shape_or_dtype_is_refused_before_anything_else(shift):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bank = cl.TrackerBank(2, lifecycle="device", max_tracks=8)
    with pytest.raises(ValueError, match=r"camera_motion: expected a float32 \[2, 2\] tensor"):
        bank.update_batch(*_dets(2), camera_motion=shift)
    with pytest.raises(ValueError, match=r"camera_motion: expected a float32 \[1, 2\] tensor"):
        bank.update_batch(*_dets(1), streams=[1], camera_motion=torch.zeros((2, 2)))
