"""GPU: cnl_augment_pixel_u8 through pixel_batch and TrainTransform.

Every comparison is an equality of canvas BYTES against tests/pixel_ref.py (the rule is integer arithmetic), so there is no tolerance to
choose.  The kernel's tile is 8 canvas rows x at most 1024 columns (equal column tiles), and a FILTER canvas stages 256 columns at a time:
the 19 x 1060 shape spans three row blocks (8, 8, 3) and two column tiles (532 and 528 columns), each of three chunks (256, 256, 20 / 16)."""
import dataclasses

import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl
import pixel_ref
import warp_ref
from centernet_lightning_amd import _lib, pixel
from strided_io import GuardedBytes
from test_warp_host import CROWDHUMAN, MOT

pytestmark = pytest.mark.gpu

ONE = 1 << 16
HOLE_FILL = (9, 200, 77)
SHAPES = [(1, 4), (3, 8), (40, 52), (19, 1060)]
IDS = [f"{h}x{w}" for h, w in SHAPES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def images(N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def run(canvas, plan, holes=None, **kw):
    before = dev(canvas)
    out = cl.pixel_batch(before, plan, holes=holes, hole_fill=HOLE_FILL, **kw)
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == before.shape and out.data_ptr() != before.data_ptr()
    assert np.array_equal(before.cpu().numpy(), canvas)                                           # the canvas is only read
    return out.cpu().numpy()


def assert_same_bytes(got, ref):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


def heavy_taps():
    """Eight taps at the reach of the radius with negative weights: they sum to 65536 and sum |w| = 2^23 exactly."""
    neg = [(-15, -15, -1_000_000), (15, 15, -1_000_000), (-15, 15, -1_000_000), (15, -15, -1_000_000), (0, -7, -161_536)]
    pos = [(0, 0, 2_000_000), (3, 0, 2_000_000), (-2, 5, 227_072)]
    assert sum(w for _, _, w in neg + pos) == ONE and sum(abs(w) for _, _, w in neg + pos) == 1 << 23
    return neg + pos


def mixed_plan():
    """All five operations and NONE, one canvas each, plus a corner tap and the heavy filter: eight canvases."""
    plan = cl.PixelPlan.empty(8)
    plan.set_motion_blur(1, 15, (0, 3), (14, 9))
    plan.set_sharpen(2, 0.5)
    plan.set_posterize(3, 3)
    plan.set_solarize(4, 100)
    plan.set_equalize(5)
    plan.set_filter(6, [(15, -15, ONE)])
    plan.set_filter(7, heavy_taps())
    return plan.check()


# ----------------------------------------------------------------------------- every operation in one launch, on every shape
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_batch_that_mixes_all_operations(shape):
    canvas = images(8, *shape, seed=sum(shape))
    plan = mixed_plan()
    ref = pixel_ref.expected(canvas, plan)
    got = run(canvas, plan)
    assert_same_bytes(got, ref)
    assert np.array_equal(ref[0], canvas[0]) and all(not np.array_equal(ref[n], canvas[n]) for n in range(1, 8))
    # batch independence: a canvas alone gives the bytes it has within the batch, and a second run the same bytes
    for n in range(8):
        assert_same_bytes(run(canvas[n:n + 1], plan.single(n))[0], got[n])
    assert_same_bytes(run(canvas, plan), got)


# ----------------------------------------------------------------------------- FILTER
LINES = {"horizontal": lambda k: ((0, k // 2), (k - 1, k // 2)), "vertical": lambda k: ((k // 2, k - 1), (k // 2, 0)),
         "diagonal": lambda k: ((k - 1, 0), (0, k - 1)), "shallow": lambda k: ((0, 0), (k - 1, 1))}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_motion_blur_lines(shape):
    cases = [(k, name) for k in (3, 15, 31) for name in LINES]
    plan = cl.PixelPlan.empty(len(cases))
    for n, (k, name) in enumerate(cases):
        plan.set_motion_blur(n, k, *LINES[name](k))
        assert plan.n_taps[n] == k                                                                # every line spans the kernel
    canvas = images(len(cases), *shape, seed=11)
    assert_same_bytes(run(canvas, plan.check()), pixel_ref.expected(canvas, plan))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_single_taps_in_the_halo_corners_copy_reflected_pixels(shape):
    H, W = shape
    corners = [(15, 15), (15, -15), (-15, 15), (-15, -15)]
    plan = cl.PixelPlan.empty(4)
    for n, (dx, dy) in enumerate(corners):
        plan.set_filter(n, [(dx, dy, ONE)])
    canvas = images(4, H, W, seed=12)
    got = run(canvas, plan.check())
    assert_same_bytes(got, pixel_ref.expected(canvas, plan))
    for n, (dx, dy) in enumerate(corners):                                                        # ... which is a gather through r(), with numpy itself
        rows = [pixel_ref.reflect(y + dy, H) for y in range(H)]
        cols = [pixel_ref.reflect(x + dx, W) for x in range(W)]
        assert_same_bytes(got[n], canvas[n][rows][:, cols])


def test_sharpen_clamps_at_both_ends_and_the_heavy_filter_too():
    H, W = 40, 52
    y, x = np.mgrid[:H, :W]
    board = np.where((y + x) % 2 == 0, 0, 255).astype(np.uint8)
    canvas = images(4, H, W, seed=13)
    canvas[:3, :, :, 0] = board                                                                   # 0 / 255 checkerboards of one and of three pixels
    canvas[:3, :, :, 1] = np.where((y // 3 + x // 3) % 2 == 0, 255, 0)
    plan = cl.PixelPlan.empty(4)
    for n, alpha in enumerate((0.0, 0.5, 0.99)):
        plan.set_sharpen(n, alpha)
    plan.set_filter(3, heavy_taps())
    got = run(canvas, plan.check())
    assert_same_bytes(got, pixel_ref.expected(canvas, plan))
    assert_same_bytes(got[0], canvas[0])                                                          # alpha = 0 is the identity
    for n in (1, 2, 3):                                                                           # both clamps fire: the unclamped sums leave 0..255 on both sides
        taps = [tuple(int(v) for v in t) for t in plan.taps[n, :plan.n_taps[n]]]
        acc = sum(w * np.pad(canvas[n].astype(np.int64), ((15, 15), (15, 15), (0, 0)), mode="reflect")[15 + dy:15 + dy + H, 15 + dx:15 + dx + W]
                  for dx, dy, w in taps)
        assert ((acc + 32768) >> 16).min() < 0 and ((acc + 32768) >> 16).max() > 255


# ----------------------------------------------------------------------------- tables
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_posterize_and_solarize_on_a_ramp(shape):
    H, W = shape
    ramp = (np.arange(H * W * 3, dtype=np.int64) * 7 % 256).astype(np.uint8).reshape(H, W, 3)     # every value where the canvas has 256 bytes
    cases = [(pixel.POSTERIZE, b) for b in range(9)] + [(pixel.SOLARIZE, t) for t in (0, 1, 128, 255)]
    plan = cl.PixelPlan.empty(len(cases))
    for n, (op, v) in enumerate(cases):
        (plan.set_posterize if op == pixel.POSTERIZE else plan.set_solarize)(n, v)
    canvas = np.repeat(ramp[None], len(cases), axis=0)
    got = run(canvas, plan.check())
    assert_same_bytes(got, pixel_ref.expected(canvas, plan))
    assert not got[0].any() and np.array_equal(got[8], ramp) and np.array_equal(got[9], 255 - ramp)      # bits 0, bits 8, t = 0 as stated


def equalize_cases(H, W, seed):
    """random; constant; two-valued; all pixels but one in the lowest bin; channels that differ in kind."""
    rng = np.random.default_rng(seed)
    c = np.empty((5, H, W, 3), np.uint8)
    c[0] = rng.integers(0, 256, (H, W, 3))
    c[1] = (0, 131, 255)
    c[2] = np.where(rng.random((H, W, 3)) < 0.3, 40, 200)
    c[3] = (5, 0, 254)
    c[3, H // 2, W // 2] = (6, 255, 255)
    c[4, ..., 0] = rng.integers(90, 110, (H, W))
    c[4, ..., 1] = 77
    c[4, ..., 2] = np.where(rng.random((H, W)) < 0.5, 0, 1)
    return c


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_equalize_kinds_of_histograms(shape):
    canvas = equalize_cases(*shape, seed=14)
    plan = cl.PixelPlan.empty(5)
    for n in range(5):
        plan.set_equalize(n)
    ref = pixel_ref.expected(canvas, plan)
    assert_same_bytes(run(canvas, plan.check()), ref)
    assert_same_bytes(ref[1], canvas[1])                                                          # d == 0 on every channel
    assert np.array_equal(ref[4][..., 1], canvas[4][..., 1])


def test_equalize_counts_in_64_bits():
    H = W = 3000
    rng = np.random.default_rng(15)
    canvas = rng.integers(1, 256, (1, H, W, 3), dtype=np.uint8)
    canvas[0, :2, :, :] = 0                                                                       # a lowest bin of 6000 pixels
    plan = cl.PixelPlan.empty(1)
    plan.set_equalize(0)
    assert 510 * (H * W - 6000) > 2 ** 32
    assert_same_bytes(run(canvas, plan.check()), pixel_ref.expected(canvas, plan))


# ----------------------------------------------------------------------------- holes
def test_holes_are_punched_after_the_operation():
    H, W = 19, 1060
    canvas = images(8, H, W, seed=16)
    plan = mixed_plan()
    holes = np.zeros((8, 16, 4), np.int32)
    holes[:, 0] = (520, 5, 30, 6)            # across the column tiles' edge (532) and the row blocks' (8)
    holes[:, 1] = (-10, -3, 25, 8)           # over the canvas's top-left corner
    holes[:, 2] = (1050, 14, 100, 100)       # over its bottom-right corner, across the row blocks' edge (16)
    holes[:, 3] = (300, 9, 0, 5)             # a dead slot
    holes[:, 4] = (250, 0, 13, 19)           # across a chunk's edge (256), every row
    holes[:, 5] = (700, 18, 5, -1)           # dead
    holes[7] = [(30 * k + 3, k % 5 + 2, 41, 9) for k in range(16)]                                # 16 live slots that overlap
    bare = run(canvas, plan)
    got = run(canvas, plan, holes=holes)
    assert_same_bytes(got, pixel_ref.expected(canvas, plan, holes, HOLE_FILL))
    inside = np.zeros((8, H, W), bool)
    for n in range(8):
        mask = np.zeros((H, W, 3), np.uint8)
        inside[n] = pixel_ref.punch(mask, holes[n], (1, 1, 1))[..., 0] == 1
    assert inside[0].sum() == 30 * 6 + 15 * 5 + 10 * 5 + 13 * 19 and inside[7].sum() > 16 * 41 * 9 // 2
    assert (got[inside] == np.array(HOLE_FILL, np.uint8)).all() and np.array_equal(got[~inside], bare[~inside])


# ----------------------------------------------------------------------------- containment, through the C entry itself
@pytest.mark.parametrize("sentinel", [0xA5, 0x5A])
def test_only_the_output_and_the_promised_workspace_are_written(sentinel):
    N, H, W = 8, 19, 1060
    canvas = images(N, H, W, seed=17)
    plan = mixed_plan()
    holes = np.zeros((N, 16, 4), np.int32)
    holes[:, 0] = (1000, 10, 200, 200)
    lib = _lib.load()
    need = lib.cnl_augment_pixel_workspace_bytes(N, H, W)
    out = GuardedBytes(N * H * W * 3, align=4, device="cuda", sentinel=sentinel, name="out")
    space = GuardedBytes(need, align=16, device="cuda", sentinel=sentinel, name="workspace")
    records = np.zeros((N, 100), np.int32)
    plan.pack(records)
    before, d_ops, d_holes = dev(canvas), dev(records), dev(holes)
    _lib.check(lib.cnl_augment_pixel_u8(before.data_ptr(), N, H, W, d_ops.data_ptr(), plan.launches, d_holes.data_ptr(), _lib_word(HOLE_FILL), out.ptr,
                                        space.ptr, need, _lib.stream(before.device)), "cnl_augment_pixel_u8")
    torch.cuda.synchronize()
    for g in (out, space):
        ok, message = g.verdict()
        assert ok, message
    assert_same_bytes(out.result(torch.uint8, (N, H, W, 3)).numpy(), pixel_ref.expected(canvas, plan, holes, HOLE_FILL))
    assert np.array_equal(before.cpu().numpy(), canvas)
    # an overlapping output is refused, and nothing is written
    rc = lib.cnl_augment_pixel_u8(before.data_ptr(), N, H, W, d_ops.data_ptr(), plan.launches, d_holes.data_ptr(), 0, before.data_ptr() + 12, space.ptr,
                                  need, _lib.stream(before.device))
    assert rc == _lib.CNL_E_BAD_ARG and "alias" in _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(before.cpu().numpy(), canvas)


def _lib_word(fill):
    return fill[0] | fill[1] << 8 | fill[2] << 16


def test_bad_records_run_as_none_and_a_wrong_launch_mask_reads_nothing_unwritten():
    """What PixelPlan.check refuses, handed to the entry directly: every such canvas is copied."""
    N, H, W = 8, 19, 1060
    canvas = images(N, H, W, seed=18)
    plan = mixed_plan()
    plan.op[0] = 9
    plan.taps[1, 3, 0] = 16                  # an offset beyond the halo
    plan.n_taps[2] = 33
    plan.param[3] = 9
    plan.param[4] = -1
    plan.taps[6, 0, 1] = -(1 << 31)
    plan.taps[7, 0, 2] -= 1                  # sum |w| = 2^23 + 1
    records = np.zeros((N, 100), np.int32)
    plan.pack(records)
    lib = _lib.load()
    need = lib.cnl_augment_pixel_workspace_bytes(N, H, W)
    before, d_ops = dev(canvas), dev(records)
    want = canvas.copy()
    want[5] = pixel_ref.apply_op(canvas[5], pixel_ref.EQUALIZE)
    assert_same_bytes(pixel_ref.expected(canvas, plan), want)
    for launches, ref in ((3, want), (1, canvas), (0, canvas)):                                   # without the histogram EQUALIZE is the identity table
        out = torch.full((N, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
        space = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cnl_augment_pixel_u8(before.data_ptr(), N, H, W, d_ops.data_ptr(), launches, None, 0, out.data_ptr(), space.data_ptr(), need,
                                            _lib.stream(before.device)), "cnl_augment_pixel_u8")
        assert_same_bytes(out.cpu().numpy(), ref)


# ----------------------------------------------------------------------------- TrainTransform, end to end
SIZES = [(37, 53), (48, 64), (20, 31), (64, 50)]
COLOURS = dict(fill=(114, 7, 201), hole_fill=HOLE_FILL, border=(31, 150, 66))


def frames_and_targets(seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in SIZES]
    targets = []
    for (h, w) in SIZES:
        k = int(rng.integers(1, 5))
        xy = rng.uniform(0, (w * 0.7, h * 0.7), (k, 2))
        targets.append({"boxes": np.concatenate([xy, rng.uniform(3, (w * 0.3, h * 0.3), (k, 2))], axis=1), "labels": rng.integers(0, 5, k),
                        "ids": rng.integers(0, 99, k)})
    return frames, targets


def check_call(t, frames, targets):
    """One call of a TrainTransform against warp_ref followed by pixel_ref on its .last_plan, and its targets against warp_batch's."""
    canvas, out = t([dev(f) for f in frames], targets)
    plan, pix = t.last_plan
    ref = warp_ref.expected_canvas(frames, dataclasses.replace(plan, holes=np.zeros_like(plan.holes)), COLOURS["fill"], HOLE_FILL, COLOURS["border"])
    ref = pixel_ref.expected(ref, pix, plan.holes, HOLE_FILL)
    assert_same_bytes(canvas.cpu().numpy(), ref)
    _, want = cl.warp_batch([dev(f) for f in frames], plan, targets, **COLOURS)
    assert set(out) == set(want) == {"boxes", "labels", "ids", "count"} and int(out["count"].sum()) > 0
    for k in want:
        assert torch.equal(out[k], want[k]), k
    return pix


def test_train_transform_runs_the_crowdhuman_list():
    frames, targets = frames_and_targets(19)
    t = cl.TrainTransform.from_config(CROWDHUMAN, height=64, width=96, seed=3, **COLOURS)
    assert t.skipped == []
    ops = np.concatenate([check_call(t, frames, targets).op for _ in range(3)])
    assert set(ops.tolist()) == {pixel.NONE, pixel.FILTER}                                        # MotionBlur with p = 0.5: both happen


def test_train_transform_runs_trivial_augment_wide():
    frames, targets = frames_and_targets(20)
    t = cl.TrainTransform.from_config([{"name": "TrivialAugmentWide"}, {"name": "ColorJitter", "params": {"brightness": 0.4, "saturation": 0.4}},
                                       {"name": "Cutout", "params": {"num_holes": 3, "max_h_size": 9, "max_w_size": 14}}], height=64, width=96, seed=5,
                                      **COLOURS)
    ops = np.concatenate([check_call(t, frames, targets).op for _ in range(8)])
    assert {pixel.NONE, pixel.FILTER} <= set(ops.tolist()) and len(set(ops.tolist())) >= 4


def test_without_a_pixel_entry_the_bytes_are_train_warps():
    frames, targets = frames_and_targets(21)
    a = cl.TrainTransform.from_config(MOT, height=64, width=96, seed=9, **COLOURS)
    b = cl.TrainWarp.from_config(MOT, height=64, width=96, seed=9, **COLOURS)
    for _ in range(2):
        got, got_t = a([dev(f) for f in frames], targets)
        ref, ref_t = b([dev(f) for f in frames], targets)
        assert a.last_plan.pixel is None and torch.equal(got, ref) and all(torch.equal(got_t[k], ref_t[k]) for k in ref_t)
