"""No GPU: the pixel-level augmentation's host side — the properties of the rule's restatement (tests/pixel_ref.py), the taps of MotionBlur and
Sharpen, the plan (PixelPlan.check, sample_pixel), TrainTransform.from_config on the reference's transform lists, and the declarations and
argument checks of cnl_augment_pixel_u8 / cnl_augment_pixel_workspace_bytes."""
import ctypes
import os
import re

import numpy as np
import pytest

import centernet_lightning_amd as cl
import pixel_ref
from centernet_lightning_amd import _lib, pixel
from test_warp_host import CENTERNET, CROWDHUMAN, MOT, MOT_READ, SIZES, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 16


# ----------------------------------------------------------------------------- the restatement's own properties
def test_reflect_is_numpy_pad_reflect():
    for n in (2, 3, 5, 8):
        padded = np.pad(np.arange(n), 40, mode="reflect")
        assert [pixel_ref.reflect(i, n) for i in range(-40, n + 40)] == padded.tolist()
    assert [pixel_ref.reflect(i, 1) for i in range(-20, 21)] == [0] * 41


def random_filter(rng, n_taps=12, spread=3.0):
    """A valid filter: distinct offsets within +-15, signed weights that sum to 65536."""
    offs = set()
    while len(offs) < n_taps:
        offs.add((int(rng.integers(-15, 16)), int(rng.integers(-15, 16))))
    w = rng.integers(-int(spread * ONE / n_taps), int(spread * ONE / n_taps), n_taps)
    w[0] += ONE - w.sum()
    return [(dx, dy, int(v)) for (dx, dy), v in zip(sorted(offs), w)]


def test_a_constant_canvas_is_a_fixed_point_of_every_filter():
    rng = np.random.default_rng(0)
    for shape, value in (((5, 8), (0, 255, 17)), ((1, 4), (200, 3, 99)), ((20, 36), (255, 255, 0))):
        img = np.empty(shape + (3,), np.uint8)
        img[...] = value
        for taps in (random_filter(rng), pixel_ref.sharpen_taps(0.99), pixel_ref.line_taps(31, (0, 30), (30, 0))):
            assert sum(t[2] for t in taps) == ONE
            assert np.array_equal(pixel_ref.apply_filter(img, taps), img)


def test_posterize_and_solarize_tables():
    v = np.arange(256)
    assert np.array_equal(pixel_ref.posterize_lut(8), v) and not pixel_ref.posterize_lut(0).any()
    assert np.array_equal(pixel_ref.posterize_lut(1), np.where(v >= 128, 128, 0)) and np.array_equal(pixel_ref.posterize_lut(4), v & 0xF0)
    assert np.array_equal(pixel_ref.solarize_lut(0), 255 - v)                                     # t = 0: the full inversion
    assert np.array_equal(pixel_ref.solarize_lut(128), np.where(v >= 128, 255 - v, v))
    assert np.array_equal(pixel_ref.solarize_lut(255)[:255], v[:255]) and pixel_ref.solarize_lut(255)[255] == 0


def test_equalize_properties():
    rng = np.random.default_rng(1)
    for _ in range(20):
        lo, hi = sorted(int(x) for x in rng.integers(0, 256, 2))
        ch = rng.integers(lo, hi + 1, (int(rng.integers(1, 30)), int(rng.integers(1, 30)))).astype(np.uint8)
        lut = pixel_ref.equalize_lut(ch)
        present = np.unique(ch)
        if len(present) == 1:
            assert np.array_equal(lut, np.arange(256))                                            # d == 0: the identity
            continue
        assert lut[present[0]] == 0 and lut[present[-1]] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    img = np.zeros((4, 8, 3), np.uint8)
    img[..., 1] = 77
    img[0, 0, 2] = 9
    out = pixel_ref.apply_op(img, pixel_ref.EQUALIZE)
    assert np.array_equal(out[..., :2], img[..., :2]) and out[0, 0, 2] == 255 and out[..., 2].sum() == 255


def test_line_taps_for_every_odd_size():
    rng = np.random.default_rng(2)
    for k in range(3, 32, 2):
        ends = [((0, 0), (k - 1, k - 1)), ((0, k - 1), (k - 1, 0)), ((0, k // 2), (k - 1, k // 2)), ((k // 2, k - 1), (k // 2, 0)), ((0, 0), (k - 1, 1)),
                ((1, 0), (0, k - 1)), ((0, 0), (1, 0))]
        while len(ends) < 40:
            p = tuple((int(rng.integers(0, k)), int(rng.integers(0, k))) for _ in range(2))
            if p[0] != p[1]:
                ends.append(p)
        for p1, p2 in ends:
            taps = pixel_ref.line_taps(k, p1, p2)
            assert np.array_equal(cl.motion_blur_taps(k, p1, p2), np.array(taps, np.int32))
            at = [(dx, dy) for dx, dy, _ in taps]
            r = (k - 1) // 2
            assert len(set(at)) == len(at) <= 31 and all(abs(dx) <= r and abs(dy) <= r for dx, dy in at)
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(at, at[1:]))       # 8-connected
            assert at[0] == (p1[0] - r, p1[1] - r) and at[-1] == (p2[0] - r, p2[1] - r)
            w = [t[2] for t in taps]
            assert sum(w) == ONE and max(w) - min(w) <= 1 and w == sorted(w, reverse=True)
    for bad in ((4, (0, 0), (1, 1)), (33, (0, 0), (1, 1)), (1, (0, 0), (0, 0)), (5, (0, 0), (0, 0)), (5, (0, 0), (5, 0)), (5, (-1, 0), (2, 0))):
        with pytest.raises(ValueError, match="motion blur"):
            cl.motion_blur_taps(*bad)


def test_sharpen_taps():
    assert np.array_equal(cl.sharpen_taps(0.0)[:, 2], [0, 0, 0, 0, ONE, 0, 0, 0, 0])
    for alpha in (0.0, 0.3, 0.5, 0.99, 1.0):
        t = cl.sharpen_taps(alpha)
        assert np.array_equal(t, np.array(pixel_ref.sharpen_taps(alpha), np.int32)) and t[:, 2].sum() == ONE
        a = int(np.rint(alpha * ONE))
        assert t[4].tolist() == [0, 0, ONE + 8 * a] and set(np.delete(t[:, 2], 4).tolist()) == {-a}
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            cl.sharpen_taps(bad)


# ----------------------------------------------------------------------------- the plan
def filled_plan():
    plan = cl.PixelPlan.empty(6)
    plan.set_motion_blur(1, 15, (0, 3), (14, 9))
    plan.set_sharpen(2, 0.5)
    plan.set_posterize(3, 4)
    plan.set_solarize(4, 128)
    plan.set_equalize(5)
    return plan


def test_plan_setters_and_pack_follow_the_record_layout():
    plan = filled_plan()
    assert plan.check() is plan and len(plan) == 6 and plan.op.tolist() == [0, 1, 1, 2, 3, 4] and plan.param.tolist() == [0, 0, 0, 4, 128, 0]
    assert plan.n_taps.tolist() == [0, 15, 9, 0, 0, 0] and plan.launches == pixel.HAS_TABLE | pixel.HAS_EQUALIZE
    assert cl.PixelPlan.empty(3).launches == 0 and plan.single(3).launches == pixel.HAS_TABLE and plan.single(1).launches == 0
    one = plan.single(1)
    assert len(one) == 1 and np.array_equal(one.taps[0], plan.taps[1]) and one.check() is one
    plan.set_equalize(1)                                                                          # a setter clears what the slot held
    assert plan.n_taps[1] == 0 and not plan.taps[1].any()
    plan = filled_plan()
    records = np.zeros((6, 100), np.int32)
    plan.pack(records)
    ops = (_lib.PixelOp * 6).from_buffer_copy(records.tobytes())
    for n in range(6):
        assert (ops[n].op, ops[n].param, ops[n].n_taps, ops[n].reserved) == (plan.op[n], plan.param[n], plan.n_taps[n], 0)
        assert [list(t) for t in ops[n].taps] == plan.taps[n].tolist()
    assert pixel.RECORD_WORDS * 8 == ctypes.sizeof(_lib.PixelOp) == 400 and _lib.PixelOp.taps.offset == 16


def heavy_taps(total_abs):
    """Four taps that sum to 65536 with sum |w| = total_abs."""
    half = (total_abs - ONE) // 2
    return [(0, 0, ONE + half - 7), (1, 0, 7), (-1, 0, -(half // 2)), (0, 1, -(half - half // 2))]


@pytest.mark.parametrize("change, message", [
    (lambda p: p.op.__setitem__(0, 5), "canvas 0: op 5"),
    (lambda p: p.op.__setitem__(2, -1), "canvas 2: op -1"),
    (lambda p: p.param.__setitem__(3, 9), "canvas 3: posterize bits 9"),
    (lambda p: p.param.__setitem__(3, -1), "canvas 3: posterize bits -1"),
    (lambda p: p.param.__setitem__(4, 256), "canvas 4: solarize threshold 256"),
    (lambda p: p.n_taps.__setitem__(1, 33), "canvas 1: n_taps 33"),
    (lambda p: p.n_taps.__setitem__(2, 0), "canvas 2: n_taps 0"),
    (lambda p: p.taps.__setitem__((1, 3, 0), 16), "canvas 1: a tap offset lies beyond +-15"),
    (lambda p: p.taps.__setitem__((2, 8, 1), -16), "canvas 2: a tap offset lies beyond +-15"),
    (lambda p: p.taps.__setitem__((2, 4, 2), 5), "canvas 2: the weights sum to"),
    (lambda p: p.n_taps.__setitem__(1, 14), "canvas 1: the weights sum to"),
    (lambda p: p.set_filter(0, heavy_taps((1 << 23) + 2)), "canvas 0: sum |w|"),
    (lambda p: setattr(p, "taps", p.taps.astype(np.int64)), "taps must be an int32 array"),
    (lambda p: setattr(p, "param", p.param[:5]), "param must be an int32 array"),
])
def test_check_names_the_canvas(change, message):
    plan = filled_plan()
    change(plan)
    with pytest.raises(ValueError, match=re.escape(message)):
        plan.check()


def test_check_passes_the_bounds_themselves():
    plan = cl.PixelPlan.empty(2)
    plan.set_filter(0, heavy_taps(1 << 23))
    plan.set_filter(1, [(15, -15, ONE)] + [(-15 + i, 15, 0) for i in range(31)])
    assert plan.check() is plan and plan.n_taps.tolist() == [4, 32]
    with pytest.raises(ValueError, match="1..32 taps"):
        plan.set_filter(0, [(0, 0, 0)] * 33)
    # taps beyond n_taps and the fields of other operations are not judged
    plan = filled_plan()
    plan.taps[1, 20] = (99, 99, 99)
    plan.param[5] = 1000
    assert plan.check() is plan


def kinds_of(plan):
    """Per canvas what sample_pixel drew: the op, with MotionBlur and Sharpen told apart by their centre tap."""
    out = []
    for n in range(len(plan)):
        op = int(plan.op[n])
        out.append(("sharpen" if plan.n_taps[n] == 9 and plan.taps[n, 4, 2] >= ONE and (plan.taps[n, :9, 2] <= 0).sum() == 8 else "motion_blur")
                   if op == pixel.FILTER else pixel._OP_NAMES[op].lower())
    return out


def test_sample_pixel_holds_to_its_probabilities():
    rng = np.random.default_rng(3)
    every = dict(motion_blur=(3, 15), sharpen=(0.2, 0.5), posterize=(2, 8), solarize=(0, 255), equalize=True)
    for kind, value in every.items():
        assert set(kinds_of(cl.sample_pixel(50, rng, p=0.0, **{kind: value}))) == {"none"}
        plan = cl.sample_pixel(50, rng, p=1.0, **{kind: value})
        assert plan.check() is plan and set(kinds_of(plan)) == {kind}
        got = kinds_of(cl.sample_pixel(400, rng, p=0.5, **{kind: value}))
        assert set(got) == {"none", kind} and 140 <= got.count(kind) <= 260                       # 200 +- 6 sigma
    assert set(kinds_of(cl.sample_pixel(20, rng))) == {"none"}                                     # no kind given
    plan = cl.sample_pixel(200, np.random.default_rng(4), one_of=True, p=1.0, **every)
    assert plan.check() is plan and set(kinds_of(plan)) == set(every)
    got = kinds_of(cl.sample_pixel(200, np.random.default_rng(4), one_of=True, p=0.5, **every))
    assert set(got) == set(every) | {"none"} and 60 <= got.count("none") <= 140
    assert set(kinds_of(cl.sample_pixel(50, rng, one_of=True, p=0.0, **every))) == {"none"}
    # the parameters stay inside their ranges
    plan = cl.sample_pixel(300, rng, p=1.0, posterize=(2, 8))
    assert set(plan.param.tolist()) == set(range(2, 9))
    plan = cl.sample_pixel(300, rng, p=1.0, solarize=(10, 12))
    assert set(plan.param.tolist()) == {10, 11, 12}
    plan = cl.sample_pixel(300, rng, p=1.0, motion_blur=(3, 15))
    assert set(np.abs(plan.taps[..., :2]).max(axis=(1, 2)).tolist()) <= set(range(1, 8)) and np.abs(plan.taps[..., :2]).max() == 7
    assert 7 < np.abs(cl.sample_pixel(100, rng, p=1.0, motion_blur=31).taps[..., :2]).max() <= 15                # a number v: (3, v)
    plan = cl.sample_pixel(100, rng, p=1.0, sharpen=(0.25, 0.75))
    assert (plan.taps[:, 0, 2] <= -ONE // 4).all() and (plan.taps[:, 0, 2] >= -3 * ONE // 4).all()
    a = cl.sample_pixel(64, np.random.default_rng(9), one_of=True, **every)
    b = cl.sample_pixel(64, np.random.default_rng(9), one_of=True, **every)
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("op", "param", "n_taps", "taps"))


def test_sample_pixel_refuses_bad_settings():
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="one operation applies per canvas"):
        cl.sample_pixel(4, rng, motion_blur=(3, 7), equalize=True)
    for kw in (dict(motion_blur=(3, 33)), dict(motion_blur=(2, 2)), dict(motion_blur=(4, 4)), dict(motion_blur=1), dict(sharpen=(0.5, 1.5)), dict(sharpen=(-0.1, 0.5)),
               dict(posterize=9), dict(posterize=(3, 2)), dict(posterize=2.5), dict(solarize=256), dict(solarize=(-1, 5)), dict(equalize=1),
               dict(equalize=True, p=1.5), dict(equalize=True, p=True)):
        with pytest.raises(ValueError):
            cl.sample_pixel(4, rng, **kw)


# ----------------------------------------------------------------------------- TrivialAugmentWide's colour words
def test_colour_words_without_a_member_are_colour_matrix_exactly():
    rng = np.random.default_rng(5)
    assert np.array_equal(pixel.colour_words(), cl.augment.IDENTITY_Q12)
    for _ in range(100):
        b, c, s, h = rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(-0.5, 0.5)
        order = [int(v) for v in rng.permutation(4)]
        base = cl.augment.colour_matrix(b, c, s, h, order=order, contrast_center=100)
        assert np.array_equal(pixel.colour_words((b, c, s, h, order), None, 100), base)
        # a member with the neutral factor changes nothing; a brightness member after the jitter scales every word before the one rounding
        for op in (0, 1, 2):
            assert np.array_equal(pixel.colour_words((b, c, s, h, order), (op, 1.0), 100), base)
    assert pixel.colour_words(None, (cl.augment.BRIGHTNESS, 1.5)).tolist() == [6144, 0, 0, 0, 6144, 0, 0, 0, 6144, 0, 0, 0]
    assert pixel.colour_words(None, (cl.augment.CONTRAST, 0.5), 128).tolist() == [2048, 0, 0, 0, 2048, 0, 0, 0, 2048] + [64 * 4096] * 3
    grey = pixel.colour_words(None, (cl.augment.SATURATION, 0.0))
    assert grey[:9].reshape(3, 3).tolist() == [[1225, 2404, 467]] * 3 and not grey[9:].any()
    # composed in float64 BEFORE the rounding: brightness 0.3 then the member 1.7 is 0.51, not rint(rint(0.3 * 4096) * 1.7)
    assert pixel.colour_words((0.3, 1.0, 1.0, 0.0, [0, 1, 2, 3]), (cl.augment.BRIGHTNESS, 1.7))[0] == int(np.rint(0.3 * 1.7 * 4096))


def test_sample_trivial_draws_every_member():
    seen, rng = set(), np.random.default_rng(6)
    for _ in range(40):
        plan, pix, members = pixel.sample_trivial(SIZES, 64, 96, rng, crop=False, flip=0.0, brightness=0.4, cutout=(2, 8, 8))
        assert plan.check() is plan and pix.check() is pix and len(members) == len(pix) == len(plan) == len(SIZES)
        seen.update(members)
        for n, m in enumerate(members):
            fh, fw = SIZES[n]
            if m not in ("shear_x", "shear_y", "translate_x", "translate_y", "rotate"):
                assert plan.fwd[n, 0].tolist() == [96 / fw, 0, 0, 0, 64 / fh, 0]
            if m in ("shear_x", "rotate"):
                assert plan.fwd[n, 0, 1] != 0
            if m == "translate_x":                                                                 # an integer shift of the source frame
                shift = plan.fwd[n, 0, 2] / (96 / fw)
                assert abs(shift - round(shift)) < 1e-9 and abs(shift) <= 32 and plan.fwd[n, 0, 5] == 0
            want = {"sharpen": pixel.FILTER, "posterize": pixel.POSTERIZE, "solarize": pixel.SOLARIZE, "equalize": pixel.EQUALIZE}.get(m, pixel.NONE)
            assert pix.op[n] == want
            if m == "posterize":
                assert 2 <= pix.param[n] <= 8
    assert seen == set(pixel.TRIVIAL_MEMBERS) | {None}
    assert len(pixel.TRIVIAL_MEMBERS) == 12 and pixel.TRIVIAL_P == 12 / 13


# ----------------------------------------------------------------------------- the reference's transform lists
def test_from_config_reads_the_reference_lists_with_nothing_skipped():
    t = cl.TrainTransform.from_config(CROWDHUMAN, seed=4)
    assert (t.height, t.width) == (608, 1088) and t.skipped == [] and t.settings["motion_blur"] == (3, 15) and t.settings["pixel_p"] == 0.5
    assert {k: v for k, v in t.settings.items() if k not in ("motion_blur", "pixel_p")} == MOT_READ
    warp_plan, pixel_plan = t.sample(SIZES)
    assert warp_plan.check() is warp_plan and pixel_plan.check() is pixel_plan and len(pixel_plan) == len(SIZES) and t.last_plan.pixel is pixel_plan
    with pytest.raises(ValueError, match="MotionBlur"):                                            # TrainWarp still refuses it
        cl.TrainWarp.from_config(CROWDHUMAN)
    t = cl.TrainTransform.from_config([{"name": "TrivialAugmentWide"}], height=64, width=96)
    assert t.trivial and t.skipped == [] and t.settings["trivial_augment"] is True
    warp_plan, pixel_plan = t.sample(SIZES)
    assert warp_plan.check() is warp_plan and pixel_plan.check() is pixel_plan
    t = cl.TrainTransform.from_config(CENTERNET[:2] + [{"name": "TrivialAugmentWide"}] + CENTERNET[2:])
    assert (t.height, t.width) == (512, 512) and t.trivial and t.settings["crop"] == "random" and t.settings["brightness"] == 0.4
    assert "motion_blur=(3, 15)" in repr(cl.TrainTransform.from_config(CROWDHUMAN))


def test_without_a_pixel_entry_the_plan_is_train_warps():
    a, b = cl.TrainTransform.from_config(MOT, seed=7), cl.TrainWarp.from_config(MOT, seed=7)
    assert a.settings == b.settings == MOT_READ and a.kinds == {} and not a.trivial
    for _ in range(3):
        plan = a.sample(SIZES)
        assert plan.pixel is None and same(plan.warp, cl.sample_warp(SIZES, b.height, b.width, b.rng, **b.settings))
    # ... and with one the warp plan of the first call is still the same draw: the pixel plan is drawn after it
    c, d = cl.TrainTransform.from_config(CROWDHUMAN, seed=7), cl.TrainWarp.from_config(MOT, seed=7)
    assert same(c.sample(SIZES).warp, cl.sample_warp(SIZES, d.height, d.width, d.rng, **d.settings))


def test_from_config_pixel_entries_and_refusals():
    size = dict(height=64, width=64)
    for entry, key, value in (({"name": "MotionBlur"}, "motion_blur", 7), ({"name": "MotionBlur", "params": {"blur_limit": 9, "p": 1.0}}, "motion_blur", 9),
                              ({"name": "Sharpen", "params": {"alpha": [0, 0.99], "lightness": [1, 1]}}, "sharpen", (0, 0.99)),
                              ({"name": "Sharpen", "params": {"lightness": 1}}, "sharpen", (0.2, 0.5)),
                              ({"name": "Posterize", "params": {"num_bits": [2, 8]}}, "posterize", (2, 8)), ({"name": "Posterize"}, "posterize", 4),
                              ({"name": "Solarize", "params": {"threshold": [0, 255]}}, "solarize", (0, 255)), ({"name": "Solarize"}, "solarize", 128),
                              ({"name": "Equalize", "params": {"mode": "cv", "by_channels": True, "p": 0.25}}, "equalize", True)):
        t = cl.TrainTransform.from_config([entry], **size)
        assert t.settings[key] == value and t.settings["pixel_p"] == entry.get("params", {}).get("p", 0.5) and list(t.kinds) == [key]
        plan = t.sample(SIZES).pixel
        assert plan.check() is plan
    with pytest.raises(ValueError, match="2 pixel-level transforms .MotionBlur, Equalize."):
        cl.TrainTransform.from_config([{"name": "MotionBlur"}, {"name": "HorizontalFlip"}, {"name": "Equalize"}], **size)
    with pytest.raises(ValueError, match="one operation"):
        cl.TrainTransform.from_config([{"name": "TrivialAugmentWide"}, {"name": "Solarize"}], unsupported="skip", **size)
    for lightness in ([0.5, 1.0], 0.5, [1, 2], None):
        params = {"alpha": [0.2, 0.5]}
        if lightness is not None:
            params["lightness"] = lightness
        with pytest.raises(ValueError, match="lightness"):
            cl.TrainTransform.from_config([{"name": "Sharpen", "params": params}], **size)
    for entry, word in (({"name": "Equalize", "params": {"mode": "pil"}}, "mode"), ({"name": "Equalize", "params": {"by_channels": False}}, "by_channels"),
                        ({"name": "MotionBlur", "params": {"allow_shifted": True}}, "allow_shifted"),
                        ({"name": "TrivialAugmentWide", "params": {"p": 1}}, "TrivialAugmentWide"), ({"name": "PadIfNeeded"}, "PadIfNeeded")):
        with pytest.raises(ValueError, match=word):
            cl.TrainTransform.from_config([entry], **size)
    assert cl.TrainTransform.from_config([{"name": "PadIfNeeded"}, {"name": "Equalize"}], unsupported="skip", **size).skipped == ["PadIfNeeded"]
    with pytest.raises(ValueError, match="one operation"):
        cl.TrainTransform(64, 64, equalize=True, posterize=4)
    for kw in (dict(motion_blur=(3, 99)), dict(pixel_p=2), dict(trivial_augment=1), dict(angle=10), dict(width=62)):
        with pytest.raises(ValueError):
            cl.TrainTransform(**dict(dict(height=64, width=64), **kw))
    t = cl.TrainTransform(64, 64, hole_fill=(1, 2, 3), equalize=True)
    t.hole_fill = (4, 5, 6)
    assert t.hole_fill == t._warp.hole_fill == (4, 5, 6)


# ----------------------------------------------------------------------------- the C entries
def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint\s+cnl_augment_pixel_u8\s*\(", header) and re.search(r"\bsize_t\s+cnl_augment_pixel_workspace_bytes\s*\(", header)
    for entry in ("cnl_augment_pixel_u8", "cnl_augment_pixel_workspace_bytes"):
        assert entry in _lib.EXPORTED_SYMBOLS and hasattr(lib, entry)
    assert "typedef struct cnl_pixel_op" in header
    for phrase in ("+ 32768) >> 16", "BORDER_REFLECT_101", "(510 * cum(v) + d) / (2 d)", "v & (0xFF << (8 - bits)) & 0xFF", "v >= t ? 255 - v : v",
                   "run as NONE", "must not overlap"):
        assert phrase in header, phrase
    for name, value in (("NONE", 0), ("FILTER", 1), ("POSTERIZE", 2), ("SOLARIZE", 3), ("EQUALIZE", 4), ("MAX_TAPS", 32), ("MAX_RADIUS", 15),
                        ("HAS_TABLE", 1), ("HAS_EQUALIZE", 2)):
        assert re.search(rf"#define CNL_PIXEL_{name} {value}\b", header) and getattr(pixel, name) == getattr(pixel_ref, name, value) == value
    assert lib.cnl_version() == _lib.ABI_VERSION == 13                # new entry points and a new record only: no ABI bump
    for name in ("pixel_batch", "sample_pixel", "PixelPlan", "TrainTransform", "motion_blur_taps", "sharpen_taps"):
        assert name in cl.__all__ and hasattr(cl, name)
    makefile = open(os.path.join(ROOT, "centernet-lightning_amd", "csrc", "Makefile")).read()
    assert "augment_pixel.hip" in makefile and os.path.exists(os.path.join(ROOT, "centernet-lightning_amd", "csrc", "augment_pixel.hip"))


N_, H_, W_ = 2, 8, 12
_KEEP = {}


def host_call(lib, **change):
    """cnl_augment_pixel_u8 on (aligned) HOST buffers: every check must answer before anything is launched."""
    need = lib.cnl_augment_pixel_workspace_bytes(N_, H_, W_)
    for name, size in (("canvas", N_ * H_ * W_ * 3), ("out", N_ * H_ * W_ * 3), ("ops", N_ * 400), ("holes", N_ * 256), ("workspace", need)):
        _KEEP.setdefault(name, np.zeros(size // 8 + 4, np.int64))
    a = dict(canvas=_KEEP["canvas"].ctypes.data, N=N_, height=H_, width=W_, ops=_KEEP["ops"].ctypes.data, launches=3, holes=_KEEP["holes"].ctypes.data,
             hole_fill=0, out=_KEEP["out"].ctypes.data, workspace=_KEEP["workspace"].ctypes.data, workspace_bytes=need)
    for k, v in change.items():
        a[k] = a[k] + v[1] if isinstance(v, tuple) and v[0] == "+" else a[v[1]] + v[2] if isinstance(v, tuple) else v
    return lib.cnl_augment_pixel_u8(a["canvas"], a["N"], a["height"], a["width"], a["ops"], a["launches"], a["holes"], a["hole_fill"], a["out"],
                                    a["workspace"], a["workspace_bytes"], None)


REFUSALS = [dict(N=-1), dict(N=65536), dict(height=0), dict(height=32769), dict(width=0), dict(width=10), dict(width=32772),
            dict(height=32768, width=32768), dict(launches=4), dict(launches=-1), dict(launches=2), dict(canvas=None), dict(ops=None), dict(out=None),
            dict(workspace=None), dict(canvas=("+", 2)), dict(out=("+", 2)), dict(ops=("+", 2)), dict(holes=("+", 8)), dict(workspace=("+", 8)),
            dict(out=("=", "canvas", 0)), dict(out=("=", "canvas", 4)), dict(out=("=", "canvas", N_ * H_ * W_ * 3 - 4)), dict(canvas=("=", "out", 8))]


@pytest.mark.parametrize("change", REFUSALS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_arguments_are_refused_without_a_device(change):
    lib = _lib.load()
    assert host_call(lib, **change) == _lib.CNL_E_BAD_ARG
    assert "cnl_augment_pixel_u8" in _lib.last_error()


@pytest.mark.parametrize("delta", [-1, 1, -768, 16])
def test_the_workspace_size_must_be_exact(delta):
    lib = _lib.load()
    need = lib.cnl_augment_pixel_workspace_bytes(N_, H_, W_)
    assert host_call(lib, workspace_bytes=need + delta) == _lib.CNL_E_WORKSPACE
    assert "cnl_augment_pixel_workspace_bytes(2, 8, 12)" in _lib.last_error()


def test_an_empty_batch_is_a_no_op_without_a_device():
    lib = _lib.load()
    assert host_call(lib, N=0, canvas=None, ops=None, out=None, holes=None, workspace=None, workspace_bytes=0) == 0
    assert host_call(lib, N=0, width=10) == _lib.CNL_E_BAD_ARG                                    # ... but its canvas size is still judged


def test_workspace_query_is_a_monotone_host_function():
    q = _lib.load().cnl_augment_pixel_workspace_bytes
    assert q(1, 8, 4) == 768 + 768 * 4 and q(2, 9, 4) == 2 * (768 + 2 * 768 * 4) and q(3, 3000, 3000) == 3 * (768 + 32 * 768 * 4)
    assert q(0, 8, 8) == q(-1, 8, 8) == q(1, 0, 8) == q(1, 8, 0) == q(65536, 8, 8) == q(1, 32769, 8) == 0
    for N, H, W in ((1, 1, 4), (3, 40, 52), (32, 608, 1088), (2, 3000, 3000)):
        assert q(N, H, W) <= q(N + 1, H, W) and q(N, H, W) <= q(N, H + 1, W) and q(N, H, W) <= q(N, H, W + 4)
        assert q(N, H, W) % 16 == 0
    sizes = [q(1, h, 64) for h in range(1, 400)]
    assert sizes == sorted(sizes) and sizes[-1] == sizes[300]                                     # 32 partial histograms at the most


def test_python_surface_refuses_before_the_device():
    import torch
    plan = cl.PixelPlan.empty(1)
    canvas = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="PixelPlan"):
        cl.pixel_batch(canvas, None)
    with pytest.raises(ValueError, match="uint8"):
        cl.pixel_batch(canvas.float(), plan)
    with pytest.raises(ValueError, match="holds 1 canvases, the batch 2"):
        cl.pixel_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), plan)
    with pytest.raises(ValueError, match="holes must be an int32 array"):
        cl.pixel_batch(canvas, plan, holes=np.zeros((1, 16, 4), np.int64))
    with pytest.raises(ValueError, match="fill"):
        cl.pixel_batch(canvas, plan, hole_fill=(0, 0, 300))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        cl.pixel_batch(canvas, plan)
    plan.op[0] = 7
    with pytest.raises(ValueError, match="canvas 0: op 7"):
        cl.pixel_batch(canvas, plan)
