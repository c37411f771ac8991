"""No GPU: the augmentation plan (sample_augment, AugmentPlan.check), the colour composition and the box rule on hand-worked cases
(tests/augment_ref.py), TrainAugment.from_config on the reference's transform lists, and the declarations and argument checks of
cnl_augment_u8 / cnl_augment_boxes_f64."""
import os
import re

import numpy as np
import pytest

import augment_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(7, 5), (37, 53), (720, 1280), (1080, 1920)]
IDENTITY = [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]
JITTER = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, cutout=(10, 60, 60))


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("n_place", "frame", "window", "dest", "flip", "colour", "holes"))


# ----------------------------------------------------------------------------- the plan
def test_same_seed_same_plan_other_seed_other_plan():
    a = cl.sample_augment(SIZES, 64, 96, np.random.default_rng(5), mosaic=0.5, **JITTER)
    b = cl.sample_augment(SIZES, 64, 96, np.random.default_rng(5), mosaic=0.5, **JITTER)
    c = cl.sample_augment(SIZES, 64, 96, np.random.default_rng(6), mosaic=0.5, **JITTER)
    assert isinstance(a, cl.AugmentPlan) and same(a, b) and not same(a, c)
    assert len(a) == len(SIZES) and a.height == 64 and a.width == 96


@pytest.mark.parametrize("mosaic", [0.0, 0.5, 1.0])
def test_every_sampled_plan_passes_check(mosaic):
    seen = set()
    for seed in range(200):
        height, width = [(64, 96), (512, 512), (608, 1088), (9, 1056)][seed % 4]
        plan = cl.sample_augment(SIZES, height, width, np.random.default_rng(seed), mosaic=mosaic, **JITTER)
        assert plan.check() is plan
        seen.update(int(k) for k in plan.n_place)
        for n in range(len(plan)):
            k = int(plan.n_place[n])
            assert plan.frame[n, 0] == n
            if k == 4:                               # the quadrants tile the canvas around a centre in its middle half
                (_, _, cx, cy), (x1, _, w1, _), (_, y2, _, h2), (x3, y3, w3, h3) = plan.dest[n].tolist()
                assert cx % 4 == 0 and width / 4 - 4 <= cx <= 3 * width / 4 + 4 and height / 4 - 1 <= cy <= 3 * height / 4 + 1
                assert (x1, w1, y2, h2, x3, y3, w3, h3) == (cx, width - cx, cy, height - cy, cx, cy, width - cx, height - cy)
            else:
                assert k == 1 and plan.dest[n, 0].tolist() == [0, 0, width, height]
    assert seen == {0.0: {1}, 0.5: {1, 4}, 1.0: {4}}[mosaic]


def test_mosaic_draws_other_frames_without_replacement_when_it_can():
    for seed in range(20):
        plan = cl.sample_augment(SIZES * 2, 64, 96, np.random.default_rng(seed), mosaic=1.0)
        for n in range(len(plan)):
            assert len(set(plan.frame[n].tolist())) == 4 and plan.frame[n, 0] == n
    plan = cl.sample_augment(SIZES[:2], 64, 96, np.random.default_rng(0), mosaic=1.0)     # F < 4: with replacement
    assert plan.check() and set(plan.n_place.tolist()) == {4} and plan.frame.max() <= 1


def test_crop_false_takes_the_whole_frame_and_flip_is_a_probability():
    plan = cl.sample_augment(SIZES, 64, 96, np.random.default_rng(1), crop=False, flip=1.0)
    for n, (h, w) in enumerate(SIZES):
        assert plan.window[n, 0].tolist() == [0, 0, w, h] and plan.flip[n, 0] == 1
    assert cl.sample_augment(SIZES, 64, 96, np.random.default_rng(1), flip=0.0).flip.sum() == 0
    assert np.array_equal(plan.colour[:, 0], np.tile(IDENTITY, (len(SIZES), 1))) and plan.holes.sum() == 0


def test_window_aspect_follows_the_rectangle():
    # r in [3/4, 4/3] on a square canvas: w / h of a found window stays within the range, up to the rounding of w and h
    plan = cl.sample_augment([(1080, 1920)] * 64, 512, 512, np.random.default_rng(2), scale=(0.3, 0.5))
    r = plan.window[:, 0, 2] / plan.window[:, 0, 3]
    assert r.min() > 0.74 and r.max() < 1.35 and r.std() > 0.05
    area = plan.window[:, 0, 2] * plan.window[:, 0, 3] / (1080 * 1920)
    assert area.min() > 0.29 and area.max() < 0.51


@pytest.mark.parametrize("change, message", [
    (lambda p: p.n_place.__setitem__(1, 5), "canvas 1 has 5 placements"),
    (lambda p: p.n_place.__setitem__(0, 0), "canvas 0 has 0 placements"),
    (lambda p: p.frame.__setitem__((2, 0), 9), "canvas 2 placement 0: frame 9"),
    (lambda p: p.window.__setitem__((0, 0), (3, 0, 3, 7)), "canvas 0 placement 0: window"),
    (lambda p: p.window.__setitem__((0, 0), (0, 0, 0, 7)), "canvas 0 placement 0: window"),
    (lambda p: p.dest.__setitem__((3, 0), (2, 0, 96, 64)), "canvas 3 placement 0: rectangle"),
    (lambda p: p.dest.__setitem__((3, 0), (0, 0, 94, 64)), "canvas 3 placement 0: rectangle"),
    (lambda p: p.dest.__setitem__((3, 0), (0, 1, 96, 64)), "canvas 3 placement 0: rectangle"),
    (lambda p: p.dest.__setitem__((3, 0), (0, 0, 96, 0)), "canvas 3 placement 0: rectangle"),
    (lambda p: p.colour.__setitem__((1, 0, 4), 32768), "canvas 1 placement 0: colour"),
    (lambda p: p.colour.__setitem__((1, 0, 11), -(2 ** 21) - 1), "canvas 1 placement 0: colour"),
    (lambda p: p.flip.__setitem__((1, 0), 2), "canvas 1 placement 0: flip"),
    (lambda p: p.holes.__setitem__((2, 15), (0, 0, -1, 4)), "canvas 2 hole 15"),
    (lambda p: (p.n_place.__setitem__(0, 2), p.dest.__setitem__((0, 1), (48, 10, 8, 8)), p.window.__setitem__((0, 1), (0, 0, 1, 1))),
     "canvas 0 placement 1: its rectangle overlaps placement 0's"),
])
def test_check_names_the_canvas_and_placement(change, message):
    plan = cl.sample_augment(SIZES, 64, 96, np.random.default_rng(0))
    change(plan)
    with pytest.raises(ValueError, match=re.escape(message)):
        plan.check()


def test_sample_augment_refuses_bad_settings():
    rng = np.random.default_rng(0)
    for kw in (dict(width=94), dict(height=0), dict(width=2 ** 15 + 4), dict(mosaic=1.5), dict(flip=-0.1), dict(scale=(0.5, 0.1)),
               dict(ratio=(0.0, 1.0)), dict(hue=0.6), dict(brightness=-1), dict(cutout=(17, 8, 8)), dict(cutout=(1, 0, 8)), dict(sizes=[]),
               dict(sizes=[(0, 4)])):
        args = dict(sizes=SIZES, height=64, width=96)
        args.update(kw)
        with pytest.raises(ValueError):
            cl.sample_augment(args.pop("sizes"), args.pop("height"), args.pop("width"), rng, **args)


# ----------------------------------------------------------------------------- colour
def test_colour_known_answers():
    for make in (augment.colour_matrix, augment_ref.compose_colour):
        assert make().tolist() == IDENTITY                                            # all-zero jitter: factors 1, 1, 1 and 0 turns
        assert make(hue=0.0, order=(3,)).tolist() == IDENTITY
        q = make(brightness=1.5)
        assert q.tolist() == [6144, 0, 0, 0, 6144, 0, 0, 0, 6144, 0, 0, 0]
        q = make(saturation=0.0)
        assert q.tolist() == [1225, 2404, 467] * 3 + [0, 0, 0]
        q = make(contrast=0.0)
        assert q.tolist() == [0] * 9 + [128 * 4096] * 3
        q = make(contrast=0.0, contrast_center=100)
        assert q.tolist() == [0] * 9 + [100 * 4096] * 3
        assert np.abs(make(brightness=9.0)[:9]).max() == 32767                       # clipped, not wrapped
        assert make(brightness=2.0, contrast=0.0, order=(1, 0)).tolist() == [0] * 9 + [2 ** 20] * 3      # order: contrast first, then x 2
        assert make(brightness=2.0, contrast=0.0, order=(0, 1)).tolist() == [0] * 9 + [2 ** 19] * 3


def test_the_two_compositions_agree_on_random_draws():
    rng = np.random.default_rng(3)
    for _ in range(200):
        b, c, s = rng.uniform(0.2, 1.8, 3)
        h, order = rng.uniform(-0.5, 0.5), [int(v) for v in rng.permutation(4)]
        assert np.array_equal(augment.colour_matrix(b, c, s, h, order), augment_ref.compose_colour(b, c, s, h, order))


def test_sampled_plan_carries_the_composition_of_its_draws():
    plan = cl.sample_augment(SIZES, 64, 96, np.random.default_rng(4), brightness=0.4)      # brightness alone: a diagonal in [0.6, 1.4]
    for q in plan.colour[:, 0]:
        assert q[0] == q[4] == q[8] and 0.6 * 4096 - 1 <= q[0] <= 1.4 * 4096 + 1 and not q[[1, 2, 3, 5, 6, 7, 9, 10, 11]].any()
    assert len(set(plan.colour[:, 0, 0].tolist())) > 1


def test_half_a_hue_turn_twice_returns_a_grey_ramp():
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    q = augment_ref.compose_colour(hue=0.5)
    assert q.tolist() != IDENTITY
    once = augment_ref.apply_colour(ramp, q)
    assert np.array_equal(augment_ref.apply_colour(once, q), ramp)
    red = np.array([[200, 30, 30]], dtype=np.uint8)
    assert not np.array_equal(augment_ref.apply_colour(red, q), red)                  # ... while a colour does turn


def test_apply_colour_floors_and_clamps():
    px = np.array([[10, 20, 30]], dtype=np.uint8)
    assert augment_ref.apply_colour(px, IDENTITY).tolist() == [[10, 20, 30]]
    q = [-4096, 0, 0, 0, 8192, 0, 0, 0, 4096, 0, 0, 2047]                             # -10 -> 0; 40; 30 + (2047 + 2048) >> 12 = 30
    assert augment_ref.apply_colour(px, q).tolist() == [[0, 40, 30]]
    q = [4096, 0, 0, 0, 32767, 0, 0, 0, 4096, -6 * 4096 - 2049, 0, 2048]              # 10 - 6 - (2049 - 2048) / 4096 floors to 3
    assert augment_ref.apply_colour(px, q).tolist() == [[3, 160, 31]]                  # 20 x 32767 / 4096 = 159.995... + 0.5 floors to 160
    assert augment_ref.apply_colour(np.array([[10, 40, 30]], dtype=np.uint8), q).tolist() == [[3, 255, 31]]


# ----------------------------------------------------------------------------- the box rule, worked by hand
WINDOW, DEST = (10, 20, 40, 30), (8, 4, 80, 90)      # sx = 2, sy = 3


def test_box_known_answers():
    m = augment_ref.map_box
    assert m((10, 20, 40, 30), 0, WINDOW, DEST, 0) == (8.0, 4.0, 80.0, 90.0)                  # exactly the window -> exactly the rectangle
    assert m((15, 25, 10, 10), 0, WINDOW, DEST, 0) == (18.0, 19.0, 20.0, 30.0)
    assert m((15, 25, 10, 10), 0, WINDOW, DEST, 1) == (8.0 + 80 - 30, 19.0, 20.0, 30.0)       # mirrored: u = (50, 70)
    # half outside on the left: x 0..20 against the window's 10..50 -> u = (-20, 20), clipped to (0, 20): visibility exactly 0.5
    assert m((0, 25, 20, 10), 0, WINDOW, DEST, 0) == (8.0, 19.0, 20.0, 30.0)
    assert m((0, 25, 20, 10), 0, WINDOW, DEST, 0, min_visibility=0.5) == (8.0, 19.0, 20.0, 30.0)
    assert m((0, 25, 20, 10), 0, WINDOW, DEST, 0, min_visibility=0.51) is None
    assert m((0, 25, 20, 10), 0, WINDOW, DEST, 1) == (8.0 + 60, 19.0, 20.0, 30.0)             # the same box mirrored sticks out on the right
    # clipped area exactly min_area (a window with sx = sy = 2, so that every value is exact): 0.25 x 1 source pixels -> 0.5 x 2 canvas
    # pixels; kept at 1.0, dropped just above
    square = (10, 20, 40, 45)
    assert m((10, 20, 0.25, 1), 0, square, DEST, 0) == (8.0, 4.0, 0.5, 2.0)
    assert m((10, 20, 0.25, 1), 0, square, DEST, 0, min_area=1.0000001) is None
    assert m((10, 20, 0.125, 1), 0, square, DEST, 0) is None                                  # area 0.5
    assert m((10, 20, 0.125, 1), 0, square, DEST, 0, min_area=0.5) == (8.0, 4.0, 0.25, 2.0)
    assert m((60, 25, 10, 10), 0, WINDOW, DEST, 0) is None                                    # wholly outside: clipped width 0
    assert m((15, 25, 0, 10), 0, WINDOW, DEST, 0, min_area=0.0) is None                       # zero width is never kept
    assert m((15, 25, 10, 10), -1, WINDOW, DEST, 0) is None                                   # negative label
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in range(4):
            box = [15.0, 25.0, 10.0, 10.0]
            box[i] = bad
            assert m(box, 0, WINDOW, DEST, 0) is None and m(box, 0, WINDOW, DEST, 1) is None
    assert m((-1e308, 25, 1.7e308, 10), 0, WINDOW, DEST, 0) is None                           # the mapped corner overflows: not finite


def test_expected_boxes_compacts_stably_and_zeroes_the_rest():
    plan = cl.AugmentPlan.empty([(60, 80), (60, 80)], 96, 96, N=1)
    plan.n_place[0] = 2
    plan.frame[0, :2] = (1, 0)
    plan.window[0, :2] = (WINDOW, WINDOW)
    plan.dest[0, :2] = ((8, 4, 80, 90), (88, 0, 8, 96))
    plan.check()
    boxes = np.zeros((2, 3, 4))
    boxes[0] = [(15, 25, 10, 10), (60, 25, 10, 10), (10, 20, 40, 30)]
    boxes[1] = [(60, 25, 10, 10), (15, 25, 10, 10), (0, 0, 0, 0)]
    labels, ids = np.array([[1, 2, 3], [4, 5, 6]]), np.array([[11, 12, 13], [14, 15, 16]])
    b, l, i, c = augment_ref.expected_boxes(plan, boxes, labels, ids, np.array([3, 2], np.int32))
    assert c.tolist() == [3] and l[0].tolist() == [5, 1, 3, 0, 0, 0] and i[0].tolist() == [15, 11, 13, 0, 0, 0]
    assert b[0, 0].tolist() == [18.0, 19.0, 20.0, 30.0] and b[0, 2].tolist() == [88.0, 0.0, 8.0, 96.0] and not b[0, 3:].any()


# ----------------------------------------------------------------------------- the reference's transform lists
BASE = [{"name": "HorizontalFlip", "params": {"p": 0.5}}, {"name": "RandomResizedCrop", "params": {"height": 512, "width": 512}},
        {"name": "ColorJitter", "params": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4}}]
TRACKING = [{"name": "HorizontalFlip", "params": {"p": 0.5}}, {"name": "RandomResizedCrop", "params": {"height": 608, "width": 1088}},
            {"name": "ColorJitter", "params": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4}}]
MOT = [{"name": "HorizontalFlip", "params": {"p": 0.5}}, {"name": "Affine", "params": {"scale": [0.8, 1.25], "rotate": [-10, 10]}},
       {"name": "RandomResizedCrop", "params": {"width": 1088, "height": 608}},
       {"name": "ColorJitter", "params": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4}},
       {"name": "Cutout", "params": {"num_holes": 10, "max_w_size": 60, "max_h_size": 60}}]
VALIDATION = [{"name": "Resize", "params": {"width": 1088, "height": 608}}]


def test_from_config_reads_the_reference_lists():
    a = cl.TrainAugment.from_config(BASE)
    assert (a.height, a.width) == (512, 512) and a.skipped == []
    assert a.settings == dict(flip=0.5, crop=True, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), brightness=0.4, contrast=0.4, saturation=0.4, hue=0.0)
    a = cl.TrainAugment.from_config(TRACKING, seed=4)
    assert (a.height, a.width) == (608, 1088) and a.settings["crop"] is True
    with pytest.raises(ValueError, match="Affine"):
        cl.TrainAugment.from_config(MOT)
    a = cl.TrainAugment.from_config(MOT, unsupported="skip")
    assert a.skipped == ["Affine"] and a.settings["cutout"] == (10, 60, 60) and (a.height, a.width) == (608, 1088)
    a = cl.TrainAugment.from_config(VALIDATION)
    assert (a.height, a.width) == (608, 1088) and a.settings == dict(flip=0.0, crop=False)
    plan = cl.sample_augment(SIZES, a.height, a.width, a.rng, **a.settings)
    assert plan.flip.sum() == 0 and [w.tolist() for w in plan.window[:, 0]] == [[0, 0, w, h] for (h, w) in SIZES]


def test_from_config_other_forms_and_refusals():
    a = cl.TrainAugment.from_config([{"name": "HorizontalFlip"}, {"name": "ColorJitter", "init_args": {"brightness": 0.4}},
                                     {"name": "Normalize", "init_args": {"mean": [0.5] * 3, "std": [0.5] * 3}}], height=64, width=96)
    assert (a.height, a.width) == (64, 96) and a.settings["flip"] == 0.5 and a.settings["brightness"] == 0.4 and a.skipped == []
    a = cl.TrainAugment.from_config({"HorizontalFlip": {"p": 0.25}, "RandomResizedCrop": {"width": 608, "height": 608}}, height=512)
    assert (a.height, a.width) == (512, 608) and a.settings["flip"] == 0.25
    for name in ("RandomCrop", "SmallestMaxSize", "MotionBlur"):
        with pytest.raises(ValueError, match=name):
            cl.TrainAugment.from_config([{"name": name}], height=64, width=64)
    with pytest.raises(ValueError, match="height and width"):
        cl.TrainAugment.from_config([{"name": "HorizontalFlip"}])
    with pytest.raises(ValueError, match="unknown settings"):
        cl.TrainAugment(64, 64, rotate=10)
    with pytest.raises(ValueError):
        cl.TrainAugment(64, 62)


# ----------------------------------------------------------------------------- the C entries
def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for entry in ("cnl_augment_u8", "cnl_augment_boxes_f64"):
        assert re.search(r"\bint\s+" + entry + r"\s*\(", header), f"{entry} is not declared in include/centernet_gfx950.h"
        assert entry in _lib.EXPORTED_SYMBOLS and hasattr(lib, entry)
    assert "typedef struct cnl_augment_placement" in header
    for phrase in ("dx' = flip ? dw - 1 - dx : dx", "+ 2048) >> 12", "min_visibility * full", "compacted STABLY"):
        assert phrase in header, phrase
    assert lib.cnl_version() == _lib.ABI_VERSION == 13                # new entry points and records only: no ABI bump
    import ctypes
    assert ctypes.sizeof(_lib.AugmentPlacement) == 96 and _lib.AugmentPlacement.colour.offset == 40
    for name in ("augment_batch", "sample_augment", "AugmentPlan", "TrainAugment"):
        assert name in cl.__all__ and hasattr(cl, name)


def image_call(lib, frames=0x10000, F=2, places=0x20000, n_place=0x30000, max_place=4, holes=0x40000, out=0x50000, N=2, height=64, width=96):
    """cnl_augment_u8 with fake pointers (never dereferenced: every call made with them fails validation or is a no-op)."""
    return lib.cnl_augment_u8(frames, F, places, n_place, max_place, holes, out, N, height, width, 0, 0, None)


def boxes_call(lib, places=0x20000, n_place=0x30000, max_place=4, N=2, F=2, boxes=0x60000, labels=0x70000, ids=None, count=0x80000, Gmax=8,
               out_boxes=0x90000, out_labels=0xa0000, out_ids=None, out_count=0xb0000, Gout=32, min_area=1.0, min_visibility=0.0):
    return lib.cnl_augment_boxes_f64(places, n_place, max_place, N, F, boxes, labels, ids, count, Gmax, out_boxes, out_labels, out_ids, out_count,
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
    assert "cnl_augment_u8" in _lib.last_error()


@pytest.mark.parametrize("change", BOXES_REFUSALS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_box_arguments_are_refused_without_a_device(change):
    lib = _lib.load()
    assert boxes_call(lib, **change) == _lib.CNL_E_BAD_ARG
    assert "cnl_augment_boxes_f64" in _lib.last_error()


def test_an_empty_batch_is_a_no_op_without_a_device():
    lib = _lib.load()
    assert image_call(lib, N=0, frames=None, places=None, n_place=None, out=None, holes=None) == 0
    assert boxes_call(lib, N=0, places=None, n_place=None, boxes=None, labels=None, count=None, out_boxes=None, out_labels=None, out_count=None) == 0


def test_python_surface_refuses_before_the_device():
    import torch
    plan = cl.sample_augment([(8, 8)], 16, 16, np.random.default_rng(0))
    with pytest.raises(ValueError, match="AugmentPlan"):
        cl.augment_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], None)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        cl.augment_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], plan)
    plan.n_place[0] = 0
    with pytest.raises(ValueError, match="canvas 0"):
        cl.augment_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], plan)
