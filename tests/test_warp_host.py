"""No GPU: the affine augmentation's host side — warp_inverse and affine_matrix on known answers, the plan (sample_warp, WarpPlan.check),
the box rule on hand-worked cases (tests/warp_ref.py), TrainWarp.from_config on the reference's transform lists, and the declarations and
argument checks of cnl_augment_warp_u8 / cnl_augment_warp_boxes_f64."""
import ctypes
import os
import re

import numpy as np
import pytest

import centernet_lightning_amd as cl
import warp_ref
from centernet_lightning_amd import _lib, warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(7, 5), (37, 53), (720, 1280), (1080, 1920)]
ONE = 1 << 20
MOT_SETTINGS = dict(affine_scale=(0.8, 1.25), rotate=(-10, 10), brightness=0.4, contrast=0.4, saturation=0.4, cutout=(10, 60, 60))


# ----------------------------------------------------------------------------- warp_inverse
@pytest.mark.parametrize("inverse", [cl.warp_inverse, warp_ref.warp_inverse], ids=["package", "restatement"])
def test_warp_inverse_known_answers(inverse):
    assert inverse([1, 0, 0, 0, 1, 0]).tolist() == [ONE, 0, 0, 0, ONE, 0]                                   # identity
    assert inverse([1, 0, 5, 0, 1, -3]).tolist() == [ONE, 0, -5 * ONE, 0, ONE, 3 * ONE]                     # u = X + 5: pixel dx reads X = dx - 5
    # a quarter turn of a frame 21 wide: (u, v) = (Y, 21 - X), so X = 21 - v, Y = u; canvas pixel (dx, dy) reads pixel (20 - dy, dx)
    assert inverse([0, 1, 0, -1, 0, 21]).tolist() == [0, -ONE, 20 * ONE, ONE, 0, 0]
    assert inverse([-1, 0, 21, 0, 1, 0]).tolist() == [-ONE, 0, 20 * ONE, 0, ONE, 0]                         # the mirror: X = 20 - dx
    # a reduction by two: pixel dx covers [2 dx, 2 dx + 2), its centre is the pixel INDEX 2 dx + 0.5
    assert inverse([0.5, 0, 0, 0, 0.5, 0]).tolist() == [2 * ONE, 0, ONE // 2, 0, 2 * ONE, ONE // 2]
    assert inverse([2, 0, 0, 0, 2, 0]).tolist() == [ONE // 2, 0, -ONE // 4, 0, ONE // 2, -ONE // 4]
    for bad in ([1, 2, 0, 2, 4, 0], [0, 0, 0, 0, 0, 0], [1, 0, float("nan"), 0, 1, 0], [float("inf"), 0, 0, 0, 1, 0],
                [2.0 ** -11, 0, 0, 0, 1, 0],                     # the inverse's entry 2^31 is beyond 2^30
                [1, 0, 2.0 ** 25, 0, 1, 0]):                     # the inverse's offset 2^45 is beyond 2^44
        with pytest.raises(ValueError):
            inverse(bad)
    assert inverse([2.0 ** -10, 0, 0, 0, 1, 0])[0] == 1 << 30                                                # the bounds themselves pass


def test_the_two_inverses_agree_on_random_maps():
    rng = np.random.default_rng(1)
    for _ in range(300):
        m = cl.affine_matrix(int(rng.integers(1, 2000)), int(rng.integers(1, 2000)), rng.uniform(0.2, 4, 2), rng.uniform(-180, 180), rng.uniform(-40, 40, 2),
                             rng.uniform(-100, 100, 2))
        assert np.array_equal(cl.warp_inverse(m), warp_ref.warp_inverse(m[:2].reshape(6)))


# ----------------------------------------------------------------------------- affine_matrix
def test_affine_matrix_known_answers():
    assert np.array_equal(cl.affine_matrix(10, 20), np.eye(3))
    assert np.array_equal(cl.affine_matrix(10, 20, scale=2), [[2, 0, -10], [0, 2, -5], [0, 0, 1]])            # about the centre (10, 5)
    assert np.array_equal(cl.affine_matrix(10, 20, scale=(2, 0.5)), [[2, 0, -10], [0, 0.5, 2.5], [0, 0, 1]])
    assert np.array_equal(cl.affine_matrix(10, 20, translate=(3, -4)), [[1, 0, 3], [0, 1, -4], [0, 0, 1]])
    # counter-clockwise as seen, y down: the point right of the centre goes up; exact at the quarter turns
    quarter = cl.affine_matrix(10, 20, rotate=90)
    assert np.array_equal(quarter, [[0, 1, 5], [-1, 0, 15], [0, 0, 1]])
    assert np.array_equal(quarter @ [11, 5, 1], [10, 4, 1])
    assert np.array_equal(cl.affine_matrix(10, 20, rotate=180), [[-1, 0, 20], [0, -1, 10], [0, 0, 1]])
    assert np.array_equal(cl.affine_matrix(10, 20, rotate=-90), cl.affine_matrix(10, 20, rotate=270))
    m = cl.affine_matrix(10, 20, rotate=30)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    assert np.allclose(m[:2, :2], [[c, s], [-s, c]], rtol=0, atol=1e-15) and np.allclose(m @ [10, 5, 1], [10, 5, 1], rtol=0, atol=1e-12)
    m = cl.affine_matrix(10, 20, shear=(45, 0))                                                               # x grows with y below the centre
    assert np.allclose(m, [[1, 1, -5], [0, 1, 0], [0, 0, 1]], rtol=0, atol=1e-12)
    m = cl.affine_matrix(10, 20, shear=(0, 45))
    assert np.allclose(m, [[1, 0, 0], [1, 1, -10], [0, 0, 1]], rtol=0, atol=1e-12)
    # the order: scale first, then shear, then the turn, then the shift
    m = cl.affine_matrix(10, 20, scale=(2, 3), rotate=90, shear=(45, 0), translate=(1, 2))
    assert np.allclose(m[:2, :2], np.array([[0, 1], [-1, 0]]) @ np.array([[1, 1], [0, 1]]) @ np.diag([2, 3]), rtol=0, atol=1e-12)
    assert np.allclose(m @ [10, 5, 1], [11, 7, 1], rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------- the plan
def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("n_place", "frame", "window", "dest", "fwd", "inv", "colour", "holes"))


def test_same_seed_same_plan_other_seed_other_plan():
    a = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(5), mosaic=0.5, **MOT_SETTINGS)
    b = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(5), mosaic=0.5, **MOT_SETTINGS)
    c = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(6), mosaic=0.5, **MOT_SETTINGS)
    assert isinstance(a, cl.WarpPlan) and same(a, b) and not same(a, c)
    assert len(a) == len(SIZES) and a.height == 64 and a.width == 96 and a.fwd.dtype == np.float64 and a.inv.dtype == np.int64


@pytest.mark.parametrize("mosaic", [0.0, 0.5, 1.0])
def test_every_sampled_plan_passes_check(mosaic):
    seen = set()
    for seed in range(200):
        height, width = [(64, 96), (512, 512), (608, 1088), (9, 1056)][seed % 4]
        extra = [dict(), dict(shear={"x": (-45, 45), "y": 0}, translate_px={"x": 32, "y": 0}), dict(crop="random", smallest_max_size=512),
                 dict(crop=False, translate_percent=(-0.1, 0.1), keep_ratio=True, affine_p=0.5)][(seed // 4) % 4]
        plan = cl.sample_warp(SIZES, height, width, np.random.default_rng(seed), mosaic=mosaic, **MOT_SETTINGS, **extra)
        assert plan.check() is plan
        seen.update(int(k) for k in plan.n_place)
        for n in range(len(plan)):
            for p in range(int(plan.n_place[n])):
                fh, fw = SIZES[int(plan.frame[n, p])]
                assert plan.window[n, p].tolist() == [0, 0, fw, fh]
                assert np.array_equal(plan.inv[n, p], warp_ref.warp_inverse(plan.fwd[n, p]))
    assert seen == {0.0: {1}, 0.5: {1, 4}, 1.0: {4}}[mosaic]


def test_without_an_affine_transform_the_map_is_the_window_onto_the_rectangle():
    plan = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(1), crop=False, flip=0.0)
    for n, (h, w) in enumerate(SIZES):
        assert plan.fwd[n, 0].tolist() == [96 / w, 0, 0, 0, 64 / h, 0]
    plan = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(1), crop=False, flip=1.0)
    for n, (h, w) in enumerate(SIZES):
        assert plan.fwd[n, 0].tolist() == [-96 / w, 0, 96, 0, 64 / h, 0]                  # the mirror is folded into the map
    # SmallestMaxSize + RandomCrop: the frame scaled so that its smaller side is 64, a canvas-sized window of it at an integer offset
    plan = cl.sample_warp([(720, 1280), (30, 40)], 64, 96, np.random.default_rng(2), crop="random", smallest_max_size=64, flip=0.0)
    sx, _, tx, _, sy, ty = plan.fwd[0, 0].tolist()
    assert (sx, sy) == (114 / 1280, 64 / 720) and ty == 0 and float(tx).is_integer() and -(114 - 96) <= tx <= 0
    # without a size the frame keeps its own: a 30 x 40 frame is centred on the border (albumentations raises here)
    plan = cl.sample_warp([(30, 40)], 64, 96, np.random.default_rng(2), crop="random", flip=0.0)
    assert plan.fwd[0, 0].tolist() == [1, 0, 28, 0, 1, 17]


def test_affine_draws_stay_in_their_ranges():
    plan = cl.sample_warp([(100, 100)] * 64, 100, 100, np.random.default_rng(3), crop=False, flip=0.0, affine_scale=(0.8, 1.25), rotate=(-10, 10))
    lin = plan.fwd[:, 0].reshape(-1, 2, 3)[:, :, :2]
    sx, sy = np.hypot(lin[:, 0, 0], lin[:, 1, 0]), np.hypot(lin[:, 0, 1], lin[:, 1, 1])                  # the lengths of the columns
    angle = np.degrees(np.arctan2(lin[:, 0, 1] / sy, lin[:, 1, 1] / sy))
    assert 0.8 <= sx.min() and sx.max() <= 1.25 and 0.8 <= sy.min() and sy.max() <= 1.25 and np.abs(sx - sy).max() > 0.05
    assert -10 <= angle.min() < -3 and 3 < angle.max() <= 10
    keep = cl.sample_warp([(100, 100)] * 8, 100, 100, np.random.default_rng(3), crop=False, flip=0.0, affine_scale=(0.8, 1.25), keep_ratio=True)
    assert np.array_equal(keep.fwd[:, 0, 0], keep.fwd[:, 0, 4])
    never = cl.sample_warp([(100, 100)] * 8, 100, 100, np.random.default_rng(3), crop=False, flip=0.0, rotate=45, affine_p=0.0)
    assert np.array_equal(never.fwd[:, 0], np.tile([1.0, 0, 0, 0, 1, 0], (8, 1)))


@pytest.mark.parametrize("change, message", [
    (lambda p: p.n_place.__setitem__(1, 5), "canvas 1 has 5 placements"),
    (lambda p: p.frame.__setitem__((2, 0), 9), "canvas 2 placement 0: frame 9"),
    (lambda p: p.window.__setitem__((0, 0), (3, 0, 3, 7)), "canvas 0 placement 0: window"),
    (lambda p: p.dest.__setitem__((3, 0), (2, 0, 96, 64)), "canvas 3 placement 0: rectangle"),
    (lambda p: p.dest.__setitem__((3, 0), (0, 0, 96, 0)), "canvas 3 placement 0: rectangle"),
    (lambda p: p.fwd.__setitem__((1, 0, 2), float("nan")), "canvas 1 placement 0: forward map"),
    (lambda p: p.inv.__setitem__((1, 0, 0), (1 << 30) + 1), "canvas 1 placement 0: inverse map"),
    (lambda p: p.inv.__setitem__((2, 0, 4), -(1 << 30) - 1), "canvas 2 placement 0: inverse map"),
    (lambda p: p.inv.__setitem__((2, 0, 5), (1 << 44) + 1), "canvas 2 placement 0: inverse map"),
    (lambda p: p.inv.__setitem__((0, 0, 2), np.iinfo(np.int64).min), "canvas 0 placement 0: inverse map"),
    (lambda p: p.colour.__setitem__((1, 0, 4), 32768), "canvas 1 placement 0: colour"),
    (lambda p: p.holes.__setitem__((2, 15), (0, 0, -1, 4)), "canvas 2 hole 15"),
    (lambda p: setattr(p, "inv", p.inv.astype(np.int32)), "inv must be an int64 array"),
    (lambda p: (p.n_place.__setitem__(0, 2), p.dest.__setitem__((0, 1), (48, 10, 8, 8)), p.window.__setitem__((0, 1), (0, 0, 1, 1))),
     "canvas 0 placement 1: its rectangle overlaps placement 0's"),
])
def test_check_names_the_canvas_and_placement(change, message):
    plan = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(0), rotate=10)
    change(plan)
    with pytest.raises(ValueError, match=re.escape(message)):
        plan.check()


def test_sample_warp_refuses_bad_settings():
    rng = np.random.default_rng(0)
    for kw in (dict(width=94), dict(mosaic=1.5), dict(flip=-0.1), dict(crop="centre"), dict(affine_scale=(0.0, 1.0)), dict(affine_scale=-1),
               dict(rotate=(10, -10)), dict(shear=90), dict(shear={"z": 3}), dict(translate_px=3, translate_percent=0.1), dict(affine_p=2),
               dict(smallest_max_size=0), dict(rotate=float("nan")), dict(sizes=[])):
        args = dict(sizes=SIZES, height=64, width=96)
        args.update(kw)
        with pytest.raises(ValueError):
            cl.sample_warp(args.pop("sizes"), args.pop("height"), args.pop("width"), rng, **args)


def test_single_and_pack_follow_the_record_layout():
    plan = cl.sample_warp(SIZES, 64, 96, np.random.default_rng(4), mosaic=1.0, **MOT_SETTINGS)
    one = plan.single(2)
    assert len(one) == 1 and np.array_equal(one.inv[0], plan.inv[2]) and np.array_equal(one.fwd[0], plan.fwd[2]) and one.sizes == plan.sizes
    N = len(plan)
    places, holes, n_place = np.zeros((N * 4, 48), np.int32), np.zeros((N * 16, 4), np.int32), np.zeros(N, np.int32)
    plan.pack(places, holes, n_place)
    records = (_lib.WarpPlacement * (N * 4)).from_buffer_copy(places.tobytes())
    for n in range(N):
        for p in range(4):
            r = records[n * 4 + p]
            assert r.frame == plan.frame[n, p] and [r.x0, r.y0, r.w, r.h] == plan.window[n, p].tolist()
            assert [r.dx0, r.dy0, r.dw, r.dh] == plan.dest[n, p].tolist() and list(r.colour) == plan.colour[n, p].tolist()
            assert list(r.inv) == plan.inv[n, p].tolist() and list(r.fwd) == plan.fwd[n, p].tolist()
            assert r.reserved0 == 0 and list(r.reserved) == [0, 0]
    assert np.array_equal(n_place, plan.n_place) and np.array_equal(holes.reshape(N, 16, 4), plan.holes)


# ----------------------------------------------------------------------------- the box rule, worked by hand
DEST = (8, 4, 80, 90)


def test_box_known_answers():
    m = warp_ref.map_box
    # the window (10, 20, 40, 30) onto the rectangle: sx = 2, sy = 3 — augment_ref's worked cases come out the same
    plain = [2, 0, -20, 0, 3, -60]
    assert m((10, 20, 40, 30), 0, plain, DEST) == (8.0, 4.0, 80.0, 90.0)
    assert m((15, 25, 10, 10), 0, plain, DEST) == (18.0, 19.0, 20.0, 30.0)
    assert m((0, 25, 20, 10), 0, plain, DEST) == (8.0, 19.0, 20.0, 30.0)                      # half outside on the left: visibility 0.5
    assert m((0, 25, 20, 10), 0, plain, DEST, min_visibility=0.51) is None
    # the same placement mirrored: u = 80 - (2 X - 20)
    flipped = [-2, 0, 100, 0, 3, -60]
    assert m((15, 25, 10, 10), 0, flipped, DEST) == (8.0 + 80 - 30, 19.0, 20.0, 30.0)
    assert m((0, 25, 20, 10), 0, flipped, DEST) == (8.0 + 60, 19.0, 20.0, 30.0)
    # a quarter turn of a 92 x 80 frame (h x w) onto an 80 x 92 rectangle (h x w): (u, v) = (Y, 80 - X)
    turn, dest = [0, 1, 0, -1, 0, 80], (4, 0, 92, 80)
    assert m((10, 20, 30, 5), 0, turn, dest) == (4.0 + 20, 40.0, 5.0, 30.0)                   # u = Y: 20..25; v = 80 - X: 40..70
    assert m((70, 0, 30, 5), 0, turn, dest) == (4.0, 0.0, 5.0, 10.0)                          # X 70..100: v = -20..10, clipped to 0..10
    assert m((70, 0, 30, 5), 0, turn, dest, min_visibility=0.34) is None                      # a third of it is visible
    # a turn by 45 degrees about the origin, scaled by sqrt 2: (u, v) = (X + Y, Y - X); the enclosing box of a square is twice as large
    assert m((10, 0, 4, 4), 0, [1, 1, 0, -1, 1, 20], (0, 0, 40, 40)) == (10.0, 6.0, 8.0, 8.0)
    assert m((15, 25, 10, 10), -1, plain, DEST) is None                                       # negative label
    assert m((15, 25, 0, 10), 0, plain, DEST, min_area=0.0) is None                           # zero width is never kept
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in range(4):
            box = [15.0, 25.0, 10.0, 10.0]
            box[i] = bad
            assert m(box, 0, plain, DEST) is None
        for i in range(6):
            fwd = [2.0, 0.0, -20.0, 0.0, 3.0, -60.0]
            fwd[i] = bad
            assert m((15, 25, 10, 10), 0, fwd, DEST) is None
    assert m((-1e308, 25, 1.7e308, 10), 0, plain, DEST) is None                               # the mapped corner overflows


def test_expected_boxes_compacts_stably_and_skips_degenerate_records():
    plan = cl.WarpPlan.empty([(60, 80), (60, 80)], 96, 96, N=1)
    plan.n_place[0] = 3
    plan.frame[0, :3] = (1, 0, 0)
    plan.window[0, :3] = (0, 0, 80, 60)
    plan.dest[0, :3] = ((8, 4, 80, 90), (88, 0, 8, 96), (0, 94, 8, 2))
    plan.set_map(0, 0, [2, 0, -20, 0, 3, -60])
    plan.set_map(0, 1, [8 / 40, 0, -2, 0, 96 / 30, -64])
    plan.inv[0, 2, 0] = (1 << 30) + 1                                                         # degenerate: carries no box
    boxes = np.zeros((2, 3, 4))
    boxes[0] = [(15, 25, 10, 10), (60, 25, 10, 10), (10, 20, 40, 30)]
    boxes[1] = [(60, 25, 10, 10), (15, 25, 10, 10), (0, 0, 0, 0)]
    labels, ids = np.array([[1, 2, 3], [4, 5, 6]]), np.array([[11, 12, 13], [14, 15, 16]])
    b, l, i, c = warp_ref.expected_boxes(plan, boxes, labels, ids, np.array([3, 2], np.int32))
    assert c.tolist() == [3] and l[0].tolist() == [5, 1, 3] + [0] * 6 and i[0].tolist() == [15, 11, 13] + [0] * 6
    assert b[0, 0].tolist() == [18.0, 19.0, 20.0, 30.0] and b[0, 2].tolist() == [88.0, 0.0, 8.0, 96.0] and not b[0, 3:].any()


# ----------------------------------------------------------------------------- the reference's transform lists
MOT = [{"name": "HorizontalFlip", "params": {"p": 0.5}}, {"name": "Affine", "params": {"scale": [0.8, 1.25], "rotate": [-10, 10]}},
       {"name": "RandomResizedCrop", "params": {"width": 1088, "height": 608}},
       {"name": "ColorJitter", "params": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4}},
       {"name": "Cutout", "params": {"num_holes": 10, "max_w_size": 60, "max_h_size": 60}}]
CROWDHUMAN = {"HorizontalFlip": {"p": 0.5}, "MotionBlur": {"blur_limit": [3, 15]}, "Affine": {"scale": [0.8, 1.25], "rotate": [-10, 10]},
              "RandomResizedCrop": {"width": 1088, "height": 608}, "ColorJitter": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4},
              "Cutout": {"num_holes": 10, "max_w_size": 60, "max_h_size": 60}}
CENTERNET = [{"name": "SmallestMaxSize", "init_args": {"max_size": 512}}, {"name": "RandomCrop", "init_args": {"height": 512, "width": 512}},
             {"name": "HorizontalFlip"}, {"name": "ColorJitter", "init_args": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4}},
             {"name": "Normalize", "init_args": {"mean": [0.5, 0.5, 0.5], "std": [0.5, 0.5, 0.5]}}]
MOT_READ = dict(flip=0.5, affine_scale=(0.8, 1.25), rotate=(-10, 10), crop="resized", scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), brightness=0.4,
                contrast=0.4, saturation=0.4, hue=0.0, cutout=(10, 60, 60))


def test_from_config_reads_the_reference_lists():
    a = cl.TrainWarp.from_config(MOT, seed=4)
    assert (a.height, a.width) == (608, 1088) and a.skipped == [] and a.settings == MOT_READ
    with pytest.raises(ValueError, match="MotionBlur"):
        cl.TrainWarp.from_config(CROWDHUMAN)
    a = cl.TrainWarp.from_config(CROWDHUMAN, unsupported="skip")
    assert (a.height, a.width) == (608, 1088) and a.skipped == ["MotionBlur"] and a.settings == MOT_READ
    a = cl.TrainWarp.from_config(CENTERNET)
    assert (a.height, a.width) == (512, 512) and a.skipped == []
    assert a.settings == dict(flip=0.5, crop="random", smallest_max_size=512, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.0)
    plan = cl.sample_warp(SIZES, a.height, a.width, a.rng, **a.settings)
    assert plan.check() is plan and abs(plan.fwd[3, 0, 4]) == 512 / 1080


def test_from_config_trivial_augment_members_and_refusals():
    # datasets/transforms.py::TrivialAugmentWide's geometric members, one at a time
    for params, key, value in (({"shear": {"x": 45, "y": 0}}, "shear", {"x": 45, "y": 0}), ({"shear": {"x": 0, "y": 45}}, "shear", {"x": 0, "y": 45}),
                               ({"translate_px": {"x": 32, "y": 0}}, "translate_px", {"x": 32, "y": 0}), ({"rotate": 135}, "rotate", 135),
                               ({"translate_percent": [-0.1, 0.1], "keep_ratio": True, "p": 0.5}, "translate_percent", (-0.1, 0.1))):
        a = cl.TrainWarp.from_config([{"name": "Affine", "params": params}], height=64, width=64)
        assert a.settings[key] == value and a.settings["crop"] is False
        plan = cl.sample_warp(SIZES, 64, 64, a.rng, **a.settings)
        assert plan.check() is plan
    # ... its photometric members, and what else is not read
    for name in ("MotionBlur", "Posterize", "Solarize", "Equalize", "Sharpen", "PadIfNeeded"):
        with pytest.raises(ValueError, match=name):
            cl.TrainWarp.from_config([{"name": name}], height=64, width=64)
        assert cl.TrainWarp.from_config([{"name": name}], height=64, width=64, unsupported="skip").skipped == [name]
    with pytest.raises(ValueError, match="fit_output"):
        cl.TrainWarp.from_config([{"name": "Affine", "params": {"rotate": 10, "fit_output": True}}], height=64, width=64)
    with pytest.raises(ValueError, match="height and width"):
        cl.TrainWarp.from_config([{"name": "Affine", "params": {"rotate": 10}}])
    with pytest.raises(ValueError, match="unknown settings"):
        cl.TrainWarp(64, 64, angle=10)
    with pytest.raises(ValueError):
        cl.TrainWarp(64, 62)
    assert "rotate=10" in repr(cl.TrainWarp(64, 64, rotate=10))


# ----------------------------------------------------------------------------- the C entries
def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for entry in ("cnl_augment_warp_u8", "cnl_augment_warp_boxes_f64"):
        assert re.search(r"\bint\s+" + entry + r"\s*\(", header), f"{entry} is not declared in include/centernet_gfx950.h"
        assert entry in _lib.EXPORTED_SYMBOLS and hasattr(lib, entry)
    assert "typedef struct cnl_warp_placement" in header
    for phrase in ("a1 = (X >> 9) & 2047", "+ 2^21) >> 22", "NOT cv2.warpAffine's", "NOT the letterbox rule", "rotate_method=\"largest_box\"",
                   "u_k = (fwd[0]*X + fwd[1]*Y) + fwd[2]", "- 0.5) * 2^20"):
        assert phrase in header, phrase
    assert lib.cnl_version() == _lib.ABI_VERSION == 13                # new entry points and a new record only: no ABI bump
    W = _lib.WarpPlacement
    assert ctypes.sizeof(W) == 192 and (W.dx0.offset, W.reserved0.offset, W.colour.offset, W.inv.offset, W.fwd.offset, W.reserved.offset) == \
        (20, 36, 40, 88, 136, 184)
    for name in ("warp_batch", "sample_warp", "WarpPlan", "TrainWarp", "affine_matrix", "warp_inverse"):
        assert name in cl.__all__ and hasattr(cl, name)
    assert warp.RECORD_WORDS * 8 == 192


def image_call(lib, frames=0x10000, F=2, places=0x20000, n_place=0x30000, max_place=4, holes=0x40000, out=0x50000, N=2, height=64, width=96):
    """cnl_augment_warp_u8 with fake pointers (never dereferenced: every call made with them fails validation or is a no-op)."""
    return lib.cnl_augment_warp_u8(frames, F, places, n_place, max_place, holes, out, N, height, width, 0, 0, 0, None)


def boxes_call(lib, places=0x20000, n_place=0x30000, max_place=4, N=2, F=2, boxes=0x60000, labels=0x70000, ids=None, count=0x80000, Gmax=8,
               out_boxes=0x90000, out_labels=0xa0000, out_ids=None, out_count=0xb0000, Gout=32, min_area=1.0, min_visibility=0.0):
    return lib.cnl_augment_warp_boxes_f64(places, n_place, max_place, N, F, boxes, labels, ids, count, Gmax, out_boxes, out_labels, out_ids, out_count,
                                          Gout, min_area, min_visibility, None)


IMAGE_REFUSALS = [dict(N=-1), dict(N=65536), dict(F=-1), dict(F=65536), dict(max_place=0), dict(max_place=5), dict(height=0), dict(height=32769),
                  dict(width=0), dict(width=94), dict(width=32772), dict(height=32768, width=32768), dict(places=None), dict(n_place=None),
                  dict(out=None), dict(frames=None), dict(places=0x20004), dict(n_place=0x30002), dict(frames=0x10004), dict(out=0x50002),
                  dict(holes=0x40008)]
BOXES_REFUSALS = [dict(N=-1), dict(N=65536), dict(F=65536), dict(max_place=0), dict(max_place=5), dict(Gmax=0), dict(Gmax=65536), dict(Gout=31),
                  dict(min_area=float("nan")), dict(min_visibility=float("nan")), dict(ids=0xc0000), dict(out_ids=0xd0000), dict(places=None),
                  dict(n_place=None), dict(boxes=None), dict(labels=None), dict(count=None), dict(out_boxes=None), dict(out_labels=None),
                  dict(out_count=None), dict(boxes=0x60004), dict(labels=0x70004), dict(count=0x80002), dict(out_boxes=0x90004),
                  dict(out_labels=0xa0004), dict(out_count=0xb0002), dict(ids=0xc0004, out_ids=0xd0000), dict(ids=0xc0000, out_ids=0xd0004)]


@pytest.mark.parametrize("change", IMAGE_REFUSALS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_arguments_are_refused_without_a_device(change):
    lib = _lib.load()
    assert image_call(lib, **change) == _lib.CNL_E_BAD_ARG
    assert "cnl_augment_warp_u8" in _lib.last_error()


@pytest.mark.parametrize("change", BOXES_REFUSALS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_box_arguments_are_refused_without_a_device(change):
    lib = _lib.load()
    assert boxes_call(lib, **change) == _lib.CNL_E_BAD_ARG
    assert "cnl_augment_warp_boxes_f64" in _lib.last_error()


def test_an_empty_batch_is_a_no_op_without_a_device():
    lib = _lib.load()
    assert image_call(lib, N=0, frames=None, places=None, n_place=None, out=None, holes=None) == 0
    assert boxes_call(lib, N=0, places=None, n_place=None, boxes=None, labels=None, count=None, out_boxes=None, out_labels=None, out_count=None) == 0


def test_python_surface_refuses_before_the_device():
    import torch
    plan = cl.sample_warp([(8, 8)], 16, 16, np.random.default_rng(0), rotate=10)
    with pytest.raises(ValueError, match="WarpPlan"):
        cl.warp_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], None)
    with pytest.raises(ValueError, match="WarpPlan"):
        cl.warp_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], cl.sample_augment([(8, 8)], 16, 16, np.random.default_rng(0)))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        cl.warp_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], plan)
    plan.inv[0, 0, 1] = 1 << 31
    with pytest.raises(ValueError, match="canvas 0 placement 0: inverse map"):
        cl.warp_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], plan)
