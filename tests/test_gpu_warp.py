"""GPU: cnl_augment_warp_u8 / cnl_augment_warp_boxes_f64 through warp_batch and TrainWarp.

Every comparison is an equality: canvas BYTES, int64 labels / ids / counts and float64 box BITS against tests/warp_ref.py (the pixel rule
is integer arithmetic on a Q20 map; the box rule is single float64 operations), so there is no tolerance to choose.  The exact maps
(identity, integer translations, quarter turns, mirrors) are compared with numpy directly, not with the restatement.  Each case asserts on
the restatement's own output that it does reach what it is there for (edges crossed, taps mixed, boxes kept and dropped)."""
import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl
import warp_ref
from strided_io import GuardedBytes

pytestmark = pytest.mark.gpu

FILL, HOLE_FILL, BORDER = (114, 7, 201), (9, 200, 77), (31, 150, 66)
IDENTITY = [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]
SATURATING = [6000, -3000, 500, -2000, 7000, -1500, 300, -4000, 9000, -40 * 4096, 30 * 4096, 0]
NEGATIVE = [-4096, 0, 0, 0, -4096, 0, 0, 0, -4096, 255 * 4096, 255 * 4096, 255 * 4096]
NAN, INF = float("nan"), float("inf")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_frames(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in sizes]


def place(plan, n, frame, dest, fwd, window=None, colour=IDENTITY):
    """The next slot of canvas n: `frame` through the forward map `fwd` into the rectangle `dest`, clipped to `window` (default: the frame)."""
    p = int(plan.n_place[n])
    h, w = plan.sizes[frame]
    plan.frame[n, p], plan.dest[n, p], plan.colour[n, p] = frame, dest, colour
    plan.window[n, p] = (0, 0, w, h) if window is None else window
    plan.set_map(n, p, fwd)
    plan.n_place[n] = p + 1


def centred(fh, fw, dw, dh, **affine):
    """affine_matrix about the frame centre, then the frame centre moved onto the rectangle's centre."""
    m = cl.affine_matrix(fh, fw, **affine)
    m[0, 2] += dw / 2 - fw / 2
    m[1, 2] += dh / 2 - fh / 2
    return m


def run(frames, plan, **kw):
    canvas, targets = cl.warp_batch([dev(f) for f in frames], plan, fill=FILL, hole_fill=HOLE_FILL, border=BORDER, **kw)
    assert targets is None and canvas.dtype == torch.uint8 and canvas.is_cuda and tuple(canvas.shape) == (len(plan), plan.height, plan.width, 3)
    return canvas.cpu().numpy()


def expected(frames, plan):
    return warp_ref.expected_canvas(frames, plan, FILL, HOLE_FILL, BORDER)


def assert_same_bytes(got, ref):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


# ----------------------------------------------------------------------------- exact maps, against numpy itself
def exact_cases():
    """-> (sizes, plan, per canvas (y slice, x slice of the canvas, the image numpy puts there)): a 13 x 21 window of a 20 x 30 frame under
    the identity and an integer translation, then the whole 13 x 21 frame 1 under the four quarter turns and the two mirrors."""
    sizes = [(20, 30), (13, 21)]
    frames = make_frames(sizes, 1)
    H, W = 13, 21
    img = frames[1]
    window = (4, 3, W, H)
    cut = frames[0][3:3 + H, 4:4 + W]
    cases = [([1, 0, -4, 0, 1, -3], window, 0, (slice(0, H), slice(0, W)), cut),                 # the window's first pixel at the rectangle's
             ([1, 0, -4 + 5, 0, 1, -3 - 2], window, 0, (slice(0, H - 2), slice(5, 24)), cut[2:, :19]),     # 5 right, 2 up: leaves the rectangle
             ([1, 0, -4 - 3, 0, 1, -3 + 6], window, 0, (slice(6, 6 + H), slice(0, W - 3)), cut[:, 3:])]    # 3 left, 6 down
    turns = [[1, 0, 0, 0, 1, 0], [0, 1, 0, -1, 0, W], [-1, 0, W, 0, -1, H], [0, -1, H, 1, 0, 0]]           # np.rot90(img, k): counter-clockwise
    for k, fwd in enumerate(turns):
        r = np.rot90(img, k)
        cases.append((fwd, None, 1, (slice(0, r.shape[0]), slice(0, r.shape[1])), r))
    cases.append(([-1, 0, W, 0, 1, 0], None, 1, (slice(0, H), slice(0, W)), np.flip(img, axis=1)))
    cases.append(([1, 0, 0, 0, -1, H], None, 1, (slice(0, H), slice(0, W)), np.flip(img, axis=0)))
    plan = cl.WarpPlan.empty(sizes, 24, 24, N=len(cases))
    for n, (fwd, win, frame, _, _) in enumerate(cases):
        place(plan, n, frame, (0, 0, 24, 24), fwd, win)
    return frames, plan.check(), [(where, image) for (_, _, _, where, image) in cases]


def test_exact_maps_copy_bytes():
    frames, plan, cases = exact_cases()
    got = run(frames, plan)
    for n, (where, image) in enumerate(cases):
        ref = np.empty((24, 24, 3), np.uint8)
        ref[...] = np.array(BORDER, np.uint8)                   # where the map leaves the window
        ref[where] = image
        assert_same_bytes(got[n], ref)
    assert_same_bytes(got, expected(frames, plan))              # ... and the restatement says the same


# ----------------------------------------------------------------------------- a general map
def general_case():
    """Rotate 10 degrees, scale 1.1 x 0.9, shear 5 degrees: a 37 x 53 frame into a 56 x 34 rectangle of a 40 x 64 canvas, clipped to a window
    smaller than the frame."""
    sizes = [(37, 53)]
    plan = cl.WarpPlan.empty(sizes, 40, 64, N=1)
    place(plan, 0, 0, (4, 3, 56, 34), centred(37, 53, 56, 34, scale=(1.1, 0.9), rotate=10, shear=(5, 0)), window=(5, 4, 40, 28), colour=IDENTITY)
    return make_frames(sizes, 2), plan.check()


def check_general_case(frames, plan):
    """The case reaches what it is for, by the restatement's own account."""
    x0, y0, w, h = plan.window[0, 0].tolist()
    _, inside, sx, sy, X, Y = warp_ref.sample(frames[0], plan.window[0, 0], 56, 34, plan.inv[0, 0], BORDER)
    assert (inside == 4).mean() >= 0.25 and ((inside > 0) & (inside < 4)).mean() >= 0.05 and (inside == 0).any()
    rows, cols = (sy >= y0) & (sy + 1 < y0 + h), (sx >= x0) & (sx + 1 < x0 + w)
    crossed = {"left": (rows & (sx == x0 - 1)).any(), "right": (rows & (sx == x0 + w - 1)).any(),
               "top": (cols & (sy == y0 - 1)).any(), "bottom": (cols & (sy == y0 + h - 1)).any()}
    assert all(crossed.values()), crossed
    assert (inside == 1).any()                                  # one tap of four: a corner of the window
    assert (X < 0).any() and (Y < 0).any() and (sx < 0).any() and (sy < 0).any()
    assert ((X >> 9) & 2047).astype(bool).mean() > 0.9          # the weights are fractions, not zeros


def test_general_map_is_the_restatement():
    frames, plan = general_case()
    check_general_case(frames, plan)
    assert_same_bytes(run(frames, plan), expected(frames, plan))


# ----------------------------------------------------------------------------- a mosaic of four warped placements
SIZES_M = [(7, 5), (37, 53), (120, 200), (64, 48)]


def mosaic_plan(sizes, height, width, cx, cy, N=1, colours=(IDENTITY, SATURATING, NEGATIVE, IDENTITY)):
    """Every canvas n: frames n, n + 1, ... (mod F) turned, sheared and stretched into the four quadrants around (cx, cy)."""
    plan = cl.WarpPlan.empty(sizes, height, width, N=N)
    rects = [(0, 0, cx, cy), (cx, 0, width - cx, cy), (0, cy, cx, height - cy), (cx, cy, width - cx, height - cy)]
    for n in range(N):
        for p, (dx0, dy0, dw, dh) in enumerate(rects):
            f = (n + p) % len(sizes)
            h, w = sizes[f]
            # turned and sheared at the frame's own scale about the rectangle's centre, then stretched over most of the rectangle
            fx, fy = (0.7 + 0.1 * p) * dw / w, (1.1 - 0.1 * p) * dh / h
            stretch = np.array([[fx, 0, (1 - fx) * dw / 2], [0, fy, (1 - fy) * dh / 2], [0, 0, 1]])
            fwd = stretch @ centred(h, w, dw, dh, rotate=[17, -33, 95, 181][(n + p) % 4], shear=(3 * p, -2 * n))
            if (n + p) % 2:                      # mirrored inside the rectangle
                fwd = np.array([[-1.0, 0, dw], [0, 1, 0], [0, 0, 1]]) @ fwd
            place(plan, n, f, (dx0, dy0, dw, dh), fwd, colour=colours[(p + n) % len(colours)])
    return plan.check()


def test_mosaic_two_column_tiles_saturating_colour_and_holes():
    # 9 x 1028: one row past an 8-row block; 257 groups are two column tiles of 129 groups (516 columns).  The quadrants meet at column 520,
    # inside the second tile, and at row 5, off the 8-row grid.
    frames = make_frames(SIZES_M, 3)
    plan = mosaic_plan(SIZES_M, 9, 1028, 520, 5, N=2)
    plan.holes[0, :5] = [(510, 3, 20, 4),        # over both seams and the tile boundary
                         (1020, 6, 30, 30),      # over the canvas's right and lower edge
                         (-5, -5, 9, 8),         # over its upper left corner
                         (100, 0, 3, 9), (101, 4, 7, 2)]
    plan.holes[1, 7] = (514, 0, 4, 9)            # canvas 1: one live slot between dead ones
    plan.check()
    ref = expected(frames, plan)
    assert (ref == 0).mean() > 0.02 and (ref == 255).mean() > 0.02            # the matrices do clamp at both ends
    assert (ref[0] == np.array(HOLE_FILL, np.uint8)).all(-1).sum() > 100
    assert_same_bytes(run(frames, plan), ref)


def test_the_lower_slot_wins_and_fill_shows_between():
    sizes = [(37, 53), (64, 48)]
    frames = make_frames(sizes, 4)
    plan = cl.WarpPlan.empty(sizes, 21, 48, N=1)
    place(plan, 0, 0, (4, 2, 32, 11), centred(37, 53, 32, 11, scale=0.4, rotate=20))
    place(plan, 0, 1, (20, 7, 24, 14), centred(64, 48, 24, 14, scale=0.3, rotate=-20), colour=NEGATIVE)      # overlaps slot 0: check() refuses it
    with pytest.raises(ValueError, match="overlaps"):
        plan.check()
    plan.check = lambda: plan                    # the entry takes overlapping rectangles: the lower slot wins
    ref = expected(frames, plan)
    only0 = plan.single(0)
    only0.n_place[0] = 1
    assert_same_bytes(ref[0, 2:13, 4:36], expected(frames, only0)[0, 2:13, 4:36])
    assert (ref[0, :2] == np.array(FILL, np.uint8)).all() and (ref[0, 13:, :20] == np.array(FILL, np.uint8)).all()
    assert_same_bytes(run(frames, plan), ref)


# ----------------------------------------------------------------------------- narrow and long sources
def test_narrow_frames_and_a_long_row():
    # rows of 3, 6, 9 and 15 bytes: below, at and above the 8 bytes of one tap load; then a 90000-byte row read at its end
    sizes = [(1, 1), (2, 2), (5, 3), (3, 5), (3, 30000)]
    frames = make_frames(sizes, 5)
    plan = cl.WarpPlan.empty(sizes, 16, 32, N=6)
    for n, (h, w) in enumerate(sizes[:4]):
        place(plan, n, n, (0, 0, 32, 16), centred(h, w, 32, 16, scale=(12 / w, 7 / h), rotate=[0, 30, -20, 45][n]))
    place(plan, 4, 2, (4, 0, 24, 16), [1, 0, 10, 0, 1, 5])       # a 5 x 3 frame copied: every byte of it
    # the long frame: columns 29985 ... beyond 29999 with a slight turn, so that taps are mixed up to the last column and past it
    place(plan, 5, 4, (0, 0, 32, 16), [1.25, 0.05, -1.25 * 29980, -0.1, 4.0, 2.0 + 0.1 * 29990])
    plan.check()
    ref = expected(frames, plan)
    assert_same_bytes(ref[4, 5:10, 14:17], frames[2])
    _, inside, sx, _, _, _ = warp_ref.sample(frames[4], plan.window[5, 0], 32, 16, plan.inv[5, 0], BORDER)
    assert (sx == 29999).any() and (sx[inside == 4] >= 29995).any() and (sx > 30000).any() and (sx.min() < 29985)
    for n in range(4):                           # every small frame shows whole taps, mixed taps and the border
        inside = warp_ref.sample(frames[n], plan.window[n, 0], 32, 16, plan.inv[n, 0], BORDER)[1]
        assert (inside == 0).any() and ((inside > 0) & (inside < 4)).any() and ((inside == 4).any() or min(sizes[n]) == 1)
    assert_same_bytes(run(frames, plan), ref)


# ----------------------------------------------------------------------------- reads stay inside rows
def pitched(images, pad_value):
    """Every image as a view with row_stride > 3 w inside a buffer of pad_value, some rows and columns in on every side."""
    views = []
    for i, f in enumerate(images):
        h, w, _ = f.shape
        wide = torch.full((h + 5, w + 7 + i, 3), pad_value, dtype=torch.uint8, device="cuda")
        view = wide[2:2 + h, 3:3 + w]
        view.copy_(dev(f))
        assert view.stride(0) > 3 * w
        views.append(view)
    return views


def test_no_byte_outside_a_frame_row_is_read():
    # black images on a black border inside 0xFF padding: any padding byte that reaches a tap shows in the canvas
    sizes = [(1, 1), (2, 2), (5, 3), (3, 5), (13, 21), (9, 40)]
    plan = cl.WarpPlan.empty(sizes, 24, 64, N=2 * len(sizes))
    for n, (h, w) in enumerate(sizes):
        s = min(40 / w, 16 / h)
        place(plan, 2 * n, n, (0, 0, 64, 24), centred(h, w, 64, 24, scale=s, rotate=[10, 45, -30, 80, 135, -5][n], shear=(5, 0)))
        place(plan, 2 * n + 1, n, (0, 0, 64, 24), centred(h, w, 64, 24, scale=(-s, s), rotate=7))       # mirrored: the row's end comes first
    plan.check()
    for n in range(len(plan)):                   # the frame's four edges are crossed
        f = int(plan.frame[n, 0])
        h, w = sizes[f]
        _, inside, sx, sy, _, _ = warp_ref.sample(np.zeros((h, w, 3), np.uint8), plan.window[n, 0], 64, 24, plan.inv[n, 0], (0, 0, 0))
        touched = inside > 0
        assert (touched & (sx == -1)).any() and (touched & (sx == w - 1)).any() and (touched & (sy == -1)).any() and (touched & (sy == h - 1)).any()
    frames = pitched([np.zeros((h, w, 3), np.uint8) for (h, w) in sizes], 0xFF)
    canvas, _ = cl.warp_batch(frames, plan, fill=(0, 0, 0), border=(0, 0, 0))
    assert not canvas.any()


def test_strided_sources_and_a_guarded_canvas():
    images = make_frames(SIZES_M, 6)
    frames = pitched(images, 0xA5)
    plan = mosaic_plan(SIZES_M, 40, 96, 36, 23, N=4)
    plan.holes[1, 0] = (30, 15, 20, 12)
    guarded = GuardedBytes(4 * 40 * 96 * 3, align=4, device="cuda", name="canvas")
    out = {"canvas": guarded.typed(torch.uint8, (4, 40, 96, 3))}
    canvas, _ = cl.warp_batch(frames, plan, fill=FILL, hole_fill=HOLE_FILL, border=BORDER, out=out)
    assert canvas.data_ptr() == guarded.ptr
    ok, message = guarded.verdict()
    assert ok, message
    assert_same_bytes(guarded.result(torch.uint8, (4, 40, 96, 3)).numpy(), expected(images, plan))
    stacked = torch.stack([dev(f) for f in make_frames([(20, 28)] * 3, 7)])          # one [F, h, w, 3] tensor, and a slice of it
    inner = stacked[:, 2:18, 4:24]
    plan = cl.sample_warp([(16, 20)] * 3, 24, 32, np.random.default_rng(0), rotate=(-30, 30), affine_scale=(0.7, 1.2), shear=10)
    got, _ = cl.warp_batch(inner, plan, fill=FILL, border=BORDER)
    assert_same_bytes(got.cpu().numpy(), warp_ref.expected_canvas(list(inner.cpu().numpy()), plan, FILL, (0, 0, 0), BORDER))


# ----------------------------------------------------------------------------- boxes
SIZES_G = [(120, 200), (64, 48), (37, 53), (90, 160), (48, 64)]


def box_plan(places_per_canvas):
    """64 x 96 canvases around the centre (48, 32): every placement a turned, sheared and sometimes mirrored frame, scaled so that boxes
    fall inside, across and outside its rectangle."""
    F = len(SIZES_G)
    plan = cl.WarpPlan.empty(SIZES_G, 64, 96, N=F)
    rects = [(0, 0, 48, 32), (48, 0, 48, 32), (0, 32, 48, 32), (48, 32, 48, 32)][:places_per_canvas]
    for n in range(F):
        for p, rect in enumerate(rects):
            f = (n + p) % F
            h, w = SIZES_G[f]
            s = [1.0, 1.6, 0.8, 2.2][(n + p) % 4] * min(48 / w, 32 / h)
            fwd = centred(h, w, 48, 32, scale=(s, -s if (n + p) % 3 == 0 else s), rotate=[10, -25, 90, 137][(n + 2 * p) % 4], shear=(4 * p, 0))
            place(plan, n, f, rect, fwd)
    return plan.check()


def make_targets(Gmax, seed):
    """boxes [F, Gmax, 4] (x, y, w, h), labels, ids, count: per frame a hand-made set first, then seeded boxes in and around the frame."""
    rng = np.random.default_rng(seed)
    F = len(SIZES_G)
    boxes, labels = np.zeros((F, Gmax, 4)), rng.integers(0, 3, (F, Gmax))
    ids = rng.integers(-50, 1000, (F, Gmax))                            # ids may be negative: they are carried, not judged
    count = np.array([Gmax, 0, Gmax, Gmax - 7, Gmax // 2], np.int32)
    for f, (h, w) in enumerate(SIZES_G):
        cx, cy = rng.uniform(-0.1 * w, 1.1 * w, Gmax), rng.uniform(-0.1 * h, 1.1 * h, Gmax)
        bw, bh = rng.uniform(0.5, 0.3 * w, Gmax), rng.uniform(0.5, 0.3 * h, Gmax)
        boxes[f] = np.stack([cx - bw / 2, cy - bh / 2, bw, bh], axis=-1)
        hand = [(0, 0, w, h), (w / 2, h / 2, 0.25, 0.25),              # the whole frame; a speck at the centre
                (NAN, 8, 4, 4), (12, 8, 4, INF), (12, -INF, 4, 4),      # not finite
                (12, 8, 0, 4), (12, 8, 4, -3),                          # empty, inverted (an inverted box still has an enclosing box)
                (1e30, 8, 4, 4), (-1e308, 8, 1.7e308, 4)]               # far outside; a corner that overflows
        boxes[f, :len(hand)] = hand
        labels[f, len(hand)] = -1                                       # a negative label on an ordinary box
        labels[f, len(hand) + 1] = -(2 ** 40)
    return boxes, labels.astype(np.int64), ids.astype(np.int64), count


@pytest.fixture(scope="module", params=[(70, 4), (300, 3)], ids=["Gmax70x4", "Gmax300x3"])
def box_case(request):
    """Gmax = 70 crosses a wave, 300 a 256-box chunk; the reference is computed once per shape."""
    Gmax, k = request.param
    plan = box_plan(k)
    boxes, labels, ids, count = make_targets(Gmax, 7)
    ref = warp_ref.expected_boxes(plan, boxes, labels, ids, count)
    given = int(sum(count[int(plan.frame[n, p])] for n in range(len(plan)) for p in range(k)))
    kept = int(ref[3].sum())
    assert kept >= given / 3 and given - kept >= given / 3, (kept, given)       # a kernel that keeps or drops everything cannot pass
    assert ref[3].max() > 64 and (Gmax < 256 or ref[3].max() > 256)
    assert (ref[2] < 0).any()
    return plan, (boxes, labels, ids, count), ref, Gmax * k


@pytest.mark.parametrize("with_ids", [False, True], ids=["labels", "labels+ids"])
@pytest.mark.parametrize("form", ["device", "list"])
def test_boxes(box_case, with_ids, form):
    plan, (boxes, labels, ids, count), ref, Gout = box_case
    N = len(plan)
    frames = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for (h, w) in SIZES_G]
    if form == "device":
        targets = {"boxes": dev(boxes), "labels": dev(labels), "count": dev(count)}
        if with_ids:
            targets["ids"] = dev(ids)
    else:
        targets = [dict({"boxes": boxes[f, :count[f]], "labels": labels[f, :count[f]]}, **({"ids": ids[f, :count[f]]} if with_ids else {}))
                   for f in range(len(SIZES_G))]
    guards = {"boxes": GuardedBytes(N * Gout * 32, align=8, device="cuda", name="boxes"), "labels": GuardedBytes(N * Gout * 8, align=8, device="cuda", name="labels"),
              "count": GuardedBytes(N * 4, align=4, device="cuda", name="count")}
    if with_ids:
        guards["ids"] = GuardedBytes(N * Gout * 8, align=8, device="cuda", name="ids")
    shapes = {"boxes": (torch.float64, (N, Gout, 4)), "labels": (torch.int64, (N, Gout)), "ids": (torch.int64, (N, Gout)), "count": (torch.int32, (N,))}
    out = {name: g.typed(*shapes[name]) for name, g in guards.items()}
    _, got = cl.warp_batch(frames, plan, targets, out=out)
    assert set(got) == set(guards) and all(got[name].data_ptr() == g.ptr for name, g in guards.items())
    for g in guards.values():
        ok, message = g.verdict()
        assert ok, message
    rb, rl, ri, rc = ref
    c = guards["count"].result(*shapes["count"]).numpy()
    assert np.array_equal(c, rc), (c, rc)
    b = guards["boxes"].result(*shapes["boxes"]).numpy()
    bad = np.argwhere(b.view(np.uint64) != rb.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), b[tuple(bad[0])], rb[tuple(bad[0])])
    assert np.array_equal(guards["labels"].result(*shapes["labels"]).numpy(), rl)
    if with_ids:
        assert np.array_equal(guards["ids"].result(*shapes["ids"]).numpy(), ri)
    for n in range(N):                           # slots beyond count are exactly zero (all bits)
        assert not b[n, c[n]:].view(np.uint64).any()


def test_boxes_larger_gout_keep_settings_and_maps_that_are_not_finite(box_case):
    plan, (boxes, labels, ids, count), _, Gout = box_case
    frames = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for (h, w) in SIZES_G]
    targets = {"boxes": dev(boxes), "labels": dev(labels), "count": dev(count)}
    for kw in (dict(min_area=0.0), dict(min_area=30.0, min_visibility=0.6)):
        _, got = cl.warp_batch(frames, plan, targets, **kw)
        rb, rl, _, rc = warp_ref.expected_boxes(plan, boxes, labels, None, count, **kw)
        assert np.array_equal(got["count"].cpu().numpy(), rc) and np.array_equal(got["labels"].cpu().numpy(), rl)
        assert np.array_equal(got["boxes"].cpu().numpy().view(np.uint64), rb.view(np.uint64))
    # forward maps with entries that are not finite (check() refuses them; the entry itself drops what they map): every slot of a canvas
    broken = box_plan(int(plan.n_place[0]))
    broken.fwd[0, 0, 2], broken.fwd[1, 1, 0], broken.fwd[2, 0, 4], broken.fwd[3, :, 5] = NAN, INF, -INF, NAN
    with pytest.raises(ValueError, match="forward map"):
        broken.check()
    broken.check = lambda: broken
    _, got = cl.warp_batch(frames, broken, targets)
    rb, rl, _, rc = warp_ref.expected_boxes(broken, boxes, labels, None, count)
    whole = warp_ref.expected_boxes(plan, boxes, labels, None, count)[3]
    assert rc[3] == 0 and (rc[:3] < whole[:3]).all() and rc[4] == whole[4]
    assert np.array_equal(got["count"].cpu().numpy(), rc) and np.array_equal(got["labels"].cpu().numpy(), rl)
    assert np.array_equal(got["boxes"].cpu().numpy().view(np.uint64), rb.view(np.uint64))
    if Gout == 900:                              # four placements of 300 boxes would be 1200 slots: more than the criterion takes
        with pytest.raises(ValueError, match="Gout = 1200"):
            cl.warp_batch(frames, box_plan(4), targets)
    with pytest.raises(ValueError, match="sizes"):
        cl.warp_batch(frames[:-1] + [torch.zeros((9, 9, 3), dtype=torch.uint8, device="cuda")], plan)


# ----------------------------------------------------------------------------- properties
SIZES_H = [(37, 53), (120, 200), (7, 5), (64, 48), (90, 160), (48, 64)]


def test_same_plan_same_bytes_and_a_batch_is_its_canvases():
    frames = make_frames(SIZES_H, 8)
    tensors = [dev(f) for f in frames]
    plan = cl.sample_warp(SIZES_H, 40, 96, np.random.default_rng(9), mosaic=0.5, affine_scale=(0.8, 1.25), rotate=(-10, 10), shear=(-5, 5),
                          brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, cutout=(6, 9, 13))
    assert set(plan.n_place.tolist()) == {1, 4}
    rng = np.random.default_rng(10)
    targets = [{"boxes": np.stack([rng.uniform(0, w, 40), rng.uniform(0, h, 40), rng.uniform(1, w / 2, 40), rng.uniform(1, h / 2, 40)], axis=-1),
                "labels": rng.integers(0, 5, 40), "ids": rng.integers(0, 99, 40)} for (h, w) in SIZES_H]
    first = cl.warp_batch(tensors, plan, targets, fill=FILL, hole_fill=HOLE_FILL, border=BORDER)
    again = cl.warp_batch(tensors, plan, targets, fill=FILL, hole_fill=HOLE_FILL, border=BORDER)
    assert torch.equal(first[0], again[0]) and all(torch.equal(first[1][k].view(torch.int64) if k == "boxes" else first[1][k],
                                                               again[1][k].view(torch.int64) if k == "boxes" else again[1][k]) for k in first[1])
    assert_same_bytes(first[0].cpu().numpy(), expected(frames, plan))
    Gout = first[1]["boxes"].shape[1]
    assert Gout == 160 and int(first[1]["count"].sum()) > 40
    for n in range(len(plan)):
        canvas, t = cl.warp_batch(tensors, plan.single(n), targets, fill=FILL, hole_fill=HOLE_FILL, border=BORDER)
        assert torch.equal(canvas[0], first[0][n])
        g = t["boxes"].shape[1]                  # a single canvas of one placement has Gout = Gmax
        assert int(t["count"][0]) == int(first[1]["count"][n])
        for k in ("boxes", "labels", "ids"):
            a, b = t[k][0], first[1][k][n]
            assert torch.equal(a.view(torch.int64).reshape(g, -1), b.view(torch.int64).reshape(Gout, -1)[:g])
            assert not b.view(torch.int64).reshape(Gout, -1)[g:].any()


def test_an_empty_batch_is_a_no_op():
    tensors = [dev(f) for f in make_frames(SIZES_H[:2], 8)]
    plan = cl.WarpPlan.empty(SIZES_H[:2], 40, 96, N=0).check()
    targets = [{"boxes": np.zeros((1, 4)), "labels": np.zeros(1, np.int64)}] * 2
    canvas, t = cl.warp_batch(tensors, plan, targets)
    assert tuple(canvas.shape) == (0, 40, 96, 3) and tuple(t["boxes"].shape) == (0, 1, 4) and tuple(t["count"].shape) == (0,)


def test_a_degenerate_record_paints_nothing_and_carries_no_box():
    sizes = [(37, 53), (64, 48)]
    frames = make_frames(sizes, 11)
    tensors = [dev(f) for f in frames]
    changes = [lambda p: p.frame.__setitem__((0, 1), 2), lambda p: p.frame.__setitem__((0, 1), -1),            # no such frame
               lambda p: p.window.__setitem__((0, 1), (40, 0, 14, 37)), lambda p: p.window.__setitem__((0, 1), (0, 0, 0, 5)),      # leaves it; empty
               lambda p: p.dest.__setitem__((0, 1), (48, 0, 48, 41)), lambda p: p.dest.__setitem__((0, 1), (50, 0, 44, 40)),       # leaves the canvas; misaligned
               lambda p: p.inv.__setitem__((0, 1, 1), -(1 << 30) - 1), lambda p: p.inv.__setitem__((0, 1, 5), (1 << 44) + 1),
               lambda p: p.inv.__setitem__((0, 1, 2), np.iinfo(np.int64).min)]
    N = len(changes)
    plan = cl.WarpPlan.empty(sizes, 40, 96, N=N)
    for n in range(N):
        place(plan, n, 1, (0, 0, 48, 40), centred(64, 48, 48, 40, scale=0.7, rotate=15))
        place(plan, n, 0, (48, 0, 48, 40), centred(37, 53, 48, 40, scale=0.8, rotate=-15), colour=SATURATING)
    healthy = expected(frames, plan.check())
    single = [plan.single(n) for n in range(N)]
    for n, (one, change) in enumerate(zip(single, changes)):
        change(one)
        for name in ("frame", "window", "dest", "inv"):
            getattr(plan, name)[n] = getattr(one, name)[0]
        with pytest.raises(ValueError, match="canvas 0 placement 1"):
            one.check()
    plan.check = lambda: plan
    targets = [{"boxes": np.array([[5.0, 5, 20, 20], [30, 10, 15, 20]]), "labels": np.array([1, 2])}] * 2
    canvas, t = cl.warp_batch(tensors, plan, targets, fill=FILL, hole_fill=HOLE_FILL, border=BORDER)
    got = canvas.cpu().numpy()
    assert_same_bytes(got, expected(frames, plan))
    assert_same_bytes(got[:, :, :48], healthy[:, :, :48])                       # the other slot is painted as ever
    assert (got[:, :, 48:] == np.array(FILL, np.uint8)).all()
    rb, rl, _, rc = warp_ref.expected_boxes(plan, np.stack([d["boxes"] for d in targets]), np.stack([d["labels"] for d in targets]), None, np.array([2, 2], np.int32))
    assert np.array_equal(t["count"].cpu().numpy(), rc) and np.array_equal(t["boxes"].cpu().numpy().view(np.uint64), rb.view(np.uint64))
    # the box entry sees frame, w, h, dw, dh and inv: what it can judge carries no box (6 of the 9), the rest keeps slot 1's boxes
    assert rc.tolist() == [2, 2, 4, 2, 4, 4, 2, 2, 2]


# ----------------------------------------------------------------------------- into the criterion
MOT = [{"name": "HorizontalFlip", "params": {"p": 0.5}}, {"name": "Affine", "params": {"scale": [0.8, 1.25], "rotate": [-10, 10]}},
       {"name": "RandomResizedCrop", "params": {"width": 1088, "height": 608}},
       {"name": "ColorJitter", "params": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4}},
       {"name": "Cutout", "params": {"num_holes": 10, "max_w_size": 60, "max_h_size": 60}}]


def test_the_mot_list_feeds_the_tracking_criterion():
    sizes = [(37, 53), (120, 200), (64, 48), (90, 160)]
    frames = [dev(f) for f in make_frames(sizes, 11)]
    rng = np.random.default_rng(12)
    listed = [{"boxes": np.stack([rng.uniform(0, 0.7 * w, 12), rng.uniform(0, 0.7 * h, 12), rng.uniform(0.1 * w, 0.3 * w, 12),
                                  rng.uniform(0.1 * h, 0.3 * h, 12)], axis=-1),
               "labels": rng.integers(0, 2, 12), "ids": rng.integers(0, 20, 12)} for (h, w) in sizes]
    N = len(sizes)
    warp = cl.TrainWarp.from_config(MOT, height=64, width=64, seed=3)
    assert warp.skipped == [] and warp.settings["rotate"] == (-10, 10) and warp.settings["cutout"] == (10, 60, 60)
    canvas, targets = warp(frames, listed)
    plan = warp.last_plan
    assert tuple(canvas.shape) == (N, 64, 64, 3) and isinstance(plan, cl.WarpPlan) and (plan.fwd[:, 0, 1] != 0).all()     # every placement is turned
    assert set(targets) == {"boxes", "labels", "count", "ids"} and int(targets["count"].min()) >= 1
    assert_same_bytes(canvas.cpu().numpy(), warp_ref.expected_canvas([f.cpu().numpy() for f in frames], plan))
    g = torch.Generator().manual_seed(13)
    outputs = {"heatmap": torch.randn((N, 2, 16, 16), generator=g).cuda().requires_grad_(),
               "box_2d": (torch.rand((N, 4, 16, 16), generator=g) * 4 + 0.5).cuda().requires_grad_(),
               "reid": torch.randn((N, 8, 16, 16), generator=g).cuda().requires_grad_()}
    criterion = cl.TrackingLoss({}, cl.ReIDLoss(emb_dim=8, max_track_ids=20).cuda())
    result = criterion(outputs, targets)
    total = result["total"]
    assert bool(torch.isfinite(total)) and float(total.detach()) > 0 and int(result["skipped"].sum()) == 0
    total.backward()
    for name, t in outputs.items():
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
