"""GPU: cnl_augment_u8 / cnl_augment_boxes_f64 through augment_batch and TrainAugment.

Every comparison is an equality: canvas BYTES, int64 labels / ids / counts and float64 box BITS against tests/augment_ref.py (the pixel
rule is the integer resize plus an integer colour matrix; the box rule is single float64 operations), so there is no tolerance to choose.
Plans are built by hand where a case needs one geometry exactly, and drawn by sample_augment otherwise."""
import numpy as np
import pytest
import torch

import augment_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _frames, _gather
from strided_io import GuardedBytes

pytestmark = pytest.mark.gpu

FILL, HOLE_FILL = (114, 7, 201), (9, 200, 77)
IDENTITY = [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]
# saturating matrices: negative entries, offsets that clamp at 0 and at 255
COLOURS = [
    [6000, -3000, 500, -2000, 7000, -1500, 300, -4000, 9000, -40 * 4096, 30 * 4096, 0],
    [-4096, 0, 0, 0, -4096, 0, 0, 0, -4096, 255 * 4096, 255 * 4096, 255 * 4096],            # the negative image
    [32767, 32767, 32767, -32767, -32767, -32767, 1225, 2404, 467, -(2 ** 21), 2 ** 21, 77],  # the bounds: all 255 / all 0 / grey
    [2048, 1024, 1024, 0, 0, 4096, 4096, 0, 0, 100 * 4096 + 2047, -100 * 4096 - 2049, 2048],
]
NAN, INF = float("nan"), float("inf")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_frames(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in sizes]


def place(plan, n, frame, window, dest, flip=0, colour=IDENTITY):
    p = int(plan.n_place[n])
    plan.frame[n, p], plan.window[n, p], plan.dest[n, p], plan.flip[n, p], plan.colour[n, p] = frame, window, dest, flip, colour
    plan.n_place[n] = p + 1


def run(frames, plan, **kw):
    canvas, targets = cl.augment_batch([dev(f) for f in frames], plan, fill=FILL, hole_fill=HOLE_FILL, **kw)
    assert targets is None and canvas.dtype == torch.uint8 and canvas.is_cuda and tuple(canvas.shape) == (len(plan), plan.height, plan.width, 3)
    return canvas.cpu().numpy()


def assert_same_bytes(got, ref):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


# ----------------------------------------------------------------------------- (a), (b): one placement against the shipped letterbox
SIZES_A = [(7, 5), (37, 53), (120, 200)]
# (frame, window (x0, y0, w, h), rectangle (dx0, dy0, dw, dh)) in a 64 x 96 canvas: a tiny frame stretched over the whole canvas, a window
# with odd origins into a rectangle inside the canvas, a window that ends at the frame's last column shrunk onto the whole canvas, and a
# window two pixels wide (rows shorter than 8 bytes: the byte-load path)
CASES_A = [(0, (0, 0, 5, 7), (0, 0, 96, 64)), (1, (3, 2, 40, 30), (8, 5, 80, 50)), (2, (1, 0, 199, 120), (0, 0, 96, 64)), (0, (3, 1, 2, 5), (4, 3, 40, 30))]


def plan_a(flip):
    plan = cl.AugmentPlan.empty(SIZES_A, 64, 96, N=len(CASES_A))
    for n, (frame, window, dest) in enumerate(CASES_A):
        place(plan, n, frame, window, dest, flip)
    return plan.check()


@pytest.fixture(scope="module")
def canvas_a():
    frames = make_frames(SIZES_A, 1)
    return frames, run(frames, plan_a(0))


def test_one_placement_is_the_restatement_and_the_shipped_letterbox(canvas_a):
    frames, got = canvas_a
    assert_same_bytes(got, augment_ref.expected_canvas(frames, plan_a(0), FILL, HOLE_FILL))
    # the shipped gather on the record (h, w, new_h = dh, new_w = dw, pad_top = dy0, pad_left = dx0) of the sliced frame
    src = _frames.open_frames([dev(f) for f in frames], "rgb", "test")
    windows = [(f, y0, x0, h, w, dh, dw, dy0, dx0) for (f, (x0, y0, w, h), (dx0, dy0, dw, dh)) in CASES_A]
    plain, _ = src.records(windows)
    shipped = _gather.gather(src.device, windows, plain, 64, 96, 3, _frames.fill_word(FILL, 3)).canvas
    assert_same_bytes(got, shipped.cpu().numpy())


def test_flip_mirrors_inside_the_rectangle(canvas_a):
    frames, plain = canvas_a
    got = run(frames, plan_a(1))
    assert_same_bytes(got, augment_ref.expected_canvas(frames, plan_a(1), FILL, HOLE_FILL))
    ref = plain.copy()
    for n, (_, _, (dx0, dy0, dw, dh)) in enumerate(CASES_A):
        ref[n, dy0:dy0 + dh, dx0:dx0 + dw] = np.flip(plain[n, dy0:dy0 + dh, dx0:dx0 + dw], axis=1)
    assert_same_bytes(got, ref)
    assert (got != plain).any()


# ----------------------------------------------------------------------------- (c): mosaic
SIZES_C = [(7, 5), (37, 53), (120, 200), (64, 48)]


def mosaic_plan(sizes, height, width, cx, cy, N=1, colours=COLOURS, flips=(0, 1, 1, 0)):
    """Every canvas n: frames n, n + 1, ... (mod F) in the four quadrants around (cx, cy), windows inside each frame."""
    plan = cl.AugmentPlan.empty(sizes, height, width, N=N)
    rects = [(0, 0, cx, cy), (cx, 0, width - cx, cy), (0, cy, cx, height - cy), (cx, cy, width - cx, height - cy)]
    for n in range(N):
        for p, rect in enumerate(rects):
            f = (n + p) % len(sizes)
            h, w = sizes[f]
            window = (w // 5, h // 7, w - w // 5 - w // 9, h - h // 7 - h // 11)
            place(plan, n, f, window, rect, flips[(p + n) % 4], colours[(p + n) % len(colours)])
    return plan.check()


def test_mosaic_with_flips_and_saturating_colours():
    # centre (36, 23): the quadrants meet at a row that is no multiple of the 8-row block and a column that is a multiple of 4 only
    frames = make_frames(SIZES_C, 2)
    plan = mosaic_plan(SIZES_C, 40, 96, 36, 23, N=4)
    ref = augment_ref.expected_canvas(frames, plan, FILL, HOLE_FILL)
    assert (ref == 0).mean() > 0.05 and (ref == 255).mean() > 0.05            # the matrices do clamp at both ends
    assert_same_bytes(run(frames, plan), ref)


# ----------------------------------------------------------------------------- (d): more than one row block and column tile
def test_wide_canvas_two_tiles_two_placements_and_fill_below():
    # 9 x 1056: one row past an 8-row block; 264 groups are two column tiles of 132 groups (528 columns), so the first rectangle spans the
    # tile boundary and the two rectangles meet at column 1028 inside the second tile; the first ends at row 7: fill below it
    sizes = [(37, 53), (120, 200)]
    frames = make_frames(sizes, 3)
    plan = cl.AugmentPlan.empty(sizes, 9, 1056, N=2)
    place(plan, 0, 0, (2, 3, 50, 30), (0, 0, 1028, 7), 0, COLOURS[3])
    place(plan, 0, 1, (0, 0, 200, 120), (1028, 0, 28, 9), 1)
    place(plan, 1, 1, (7, 9, 150, 100), (0, 0, 1028, 7), 1)
    place(plan, 1, 0, (0, 0, 53, 37), (1028, 0, 28, 9), 0, COLOURS[0])
    plan.check()
    ref = augment_ref.expected_canvas(frames, plan, FILL, HOLE_FILL)
    assert (ref[:, 7:, :1028] == np.array(FILL, np.uint8)).all()
    assert_same_bytes(run(frames, plan), ref)


# ----------------------------------------------------------------------------- (e): holes
def test_holes():
    frames = make_frames(SIZES_C, 4)
    plan = mosaic_plan(SIZES_C, 40, 96, 36, 23, N=3)
    rng = np.random.default_rng(5)
    holes = [(5, 5, 1, 1),                       # one pixel
             (6, 10, 5, 3),                      # crosses a 4-pixel group
             (34, 20, 6, 6),                     # crosses the placement boundaries at column 36 and row 23
             (50, 30, 10, 5), (55, 32, 10, 6),   # two overlapping
             (-3, -2, 8, 6), (90, 36, 20, 20),   # partly outside the canvas
             (0, 39, 96, 1)]                     # the whole last row
    holes += [(int(rng.integers(0, 92)), int(rng.integers(0, 38)), int(rng.integers(1, 5)), int(rng.integers(1, 3))) for _ in range(16 - len(holes))]
    plan.holes[0] = holes                        # all 16 slots; canvas 1: none
    plan.holes[2, 3] = (40, 8, 9, 9)             # canvas 2: live slots between dead ones (w == 0), and holes wholly outside the canvas
    plan.holes[2, 9] = (-20, 4, 10, 10)
    plan.holes[2, 12] = (20, 45, 10, 10)
    plan.holes[2, 15] = (60, 1, 3, 30)
    plan.holes[2, 5] = (10, 10, 0, 10)
    plan.check()
    ref = augment_ref.expected_canvas(frames, plan, FILL, HOLE_FILL)
    none = plan.single(1)
    assert (ref[0] == np.array(HOLE_FILL, np.uint8)).all(-1).sum() > 200
    assert_same_bytes(ref[1], augment_ref.expected_canvas(frames, none, FILL, HOLE_FILL)[0])
    assert_same_bytes(run(frames, plan), ref)


# ----------------------------------------------------------------------------- (f): strided sources, guarded canvas
def test_strided_sources_and_a_guarded_canvas():
    frames = make_frames(SIZES_C, 6)
    tensors = []
    for i, f in enumerate(frames):
        h, w, _ = f.shape
        if i % 2 == 0:                           # a row-pitched view inside a wider sentinel-filled buffer
            wide = torch.full((h, w + 11, 3), 0xA5, dtype=torch.uint8, device="cuda")
            view = wide[:, 5:5 + w]
        else:                                    # a slice of a larger [H, W, 3] tensor
            wide = torch.full((h + 13, w + 6, 3), 0x5A, dtype=torch.uint8, device="cuda")
            view = wide[9:9 + h, 2:2 + w]
        view.copy_(dev(f))
        assert not view.is_contiguous() or w == wide.shape[1]
        tensors.append(view)
    plan = mosaic_plan(SIZES_C, 40, 96, 36, 23, N=4)
    plan.holes[1, 0] = (30, 15, 20, 12)
    guarded = GuardedBytes(4 * 40 * 96 * 3, align=4, device="cuda", name="canvas")
    out = {"canvas": guarded.typed(torch.uint8, (4, 40, 96, 3))}
    canvas, _ = cl.augment_batch(tensors, plan, fill=FILL, hole_fill=HOLE_FILL, out=out)
    assert canvas.data_ptr() == guarded.ptr
    ok, message = guarded.verdict()
    assert ok, message
    assert_same_bytes(guarded.result(torch.uint8, (4, 40, 96, 3)).numpy(), augment_ref.expected_canvas(frames, plan, FILL, HOLE_FILL))
    # whole frames too, so that the last rows and columns of every view are read: nothing beyond them may leak into the canvas
    whole = cl.sample_augment(SIZES_C, 40, 96, np.random.default_rng(0), crop=False, flip=0.5)
    got, _ = cl.augment_batch(tensors, whole, fill=FILL)
    assert_same_bytes(got.cpu().numpy(), augment_ref.expected_canvas(frames, whole, FILL))


# ----------------------------------------------------------------------------- (g): boxes
SIZES_G = [(120, 200), (64, 48), (37, 53), (90, 160), (48, 64)]


def box_plan(places_per_canvas):
    """64 x 96 canvases around the centre (48, 32).  Canvas 0's first placement maps a 24 x 16 window onto 48 x 32 (sx = sy = 2: the
    min_area boundary boxes are exact); the other windows are halves and thirds of their frames, so that boxes fall inside, across and
    outside them."""
    F = len(SIZES_G)
    plan = cl.AugmentPlan.empty(SIZES_G, 64, 96, N=F)
    rects = [(0, 0, 48, 32), (48, 0, 48, 32), (0, 32, 48, 32), (48, 32, 48, 32)][:places_per_canvas]
    for n in range(F):
        for p, rect in enumerate(rects):
            f = (n + p) % F
            h, w = SIZES_G[f]
            window = (10, 6, 24, 16) if (n, p) == (0, 0) else [(0, 0, w // 2 + 3, h), (w // 3, h // 4, w - w // 3, h // 2), (w // 4, 0, w // 2, h - 5),
                                                               (0, h // 3, w, h - h // 3)][(n + p) % 4]
            place(plan, n, f, window, rect, (n + p) % 2)
    return plan.check()


def make_targets(Gmax, seed):
    """boxes [F, Gmax, 4] (x, y, w, h), labels, ids, count: per frame a hand-made set first (frame 0's is worked out for the window
    (10, 6, 24, 16) at scale 2), then seeded boxes with centres in and around the frame."""
    rng = np.random.default_rng(seed)
    F = len(SIZES_G)
    boxes, labels = np.zeros((F, Gmax, 4)), rng.integers(0, 3, (F, Gmax))
    ids = rng.integers(0, 1000, (F, Gmax))
    count = np.array([Gmax, 0, Gmax, Gmax - 7, Gmax // 2], np.int32)
    for f, (h, w) in enumerate(SIZES_G):
        cx, cy = rng.uniform(-0.1 * w, 1.1 * w, Gmax), rng.uniform(-0.1 * h, 1.1 * h, Gmax)
        bw, bh = rng.uniform(0.5, 0.3 * w, Gmax), rng.uniform(0.5, 0.3 * h, Gmax)
        boxes[f] = np.stack([cx - bw / 2, cy - bh / 2, bw, bh], axis=-1)
        hand = [(12, 8, 0.25, 1), (12, 8, 0.125, 1),                    # clipped area exactly 1.0 at scale 2 (kept) and 0.5 (dropped)
                (10, 6, 24, 16), (0, 0, w, h),                          # exactly the window; the whole frame
                (4, 8, 12, 4),                                          # half outside the window on the left
                (NAN, 8, 4, 4), (12, 8, 4, INF), (12, -INF, 4, 4),      # not finite
                (12, 8, 0, 4), (12, 8, 4, -3),                          # empty, inverted
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
    ref = augment_ref.expected_boxes(plan, boxes, labels, ids, count)
    given = int(sum(count[int(plan.frame[n, p])] for n in range(len(plan)) for p in range(k)))
    kept = int(ref[3].sum())
    assert kept >= given / 3 and given - kept >= given / 3, (kept, given)       # a kernel that keeps or drops everything cannot pass
    assert ref[3].max() > 64 and (Gmax < 256 or ref[3].max() > 256)
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
    _, got = cl.augment_batch(frames, plan, targets, out=out)
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


def test_boxes_refusals_and_keep_settings(box_case):
    plan, (boxes, labels, ids, count), _, Gout = box_case
    frames = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for (h, w) in SIZES_G]
    targets = {"boxes": dev(boxes), "labels": dev(labels), "count": dev(count)}
    for kw in (dict(min_area=0.0), dict(min_area=30.0, min_visibility=0.6)):
        _, got = cl.augment_batch(frames, plan, targets, **kw)
        rb, rl, _, rc = augment_ref.expected_boxes(plan, boxes, labels, None, count, **kw)
        assert np.array_equal(got["count"].cpu().numpy(), rc) and np.array_equal(got["labels"].cpu().numpy(), rl)
        assert np.array_equal(got["boxes"].cpu().numpy().view(np.uint64), rb.view(np.uint64))
    if Gout == 900:                              # four placements of 300 boxes would be 1200 slots: more than the criterion takes
        with pytest.raises(ValueError, match="Gout = 1200"):
            cl.augment_batch(frames, box_plan(4), targets)
    with pytest.raises(ValueError, match="targets 'labels'"):
        cl.augment_batch(frames, plan, dict(targets, labels=targets["labels"].int()))
    with pytest.raises(ValueError, match="sizes"):
        cl.augment_batch(frames[:-1] + [torch.zeros((9, 9, 3), dtype=torch.uint8, device="cuda")], plan)


# ----------------------------------------------------------------------------- (h): determinism, independence of the canvases
def test_same_plan_same_bytes_and_a_batch_is_its_canvases():
    sizes = [(37, 53), (120, 200), (7, 5), (64, 48), (90, 160), (48, 64)]
    frames = make_frames(sizes, 8)
    tensors = [dev(f) for f in frames]
    plan = cl.sample_augment(sizes, 40, 96, np.random.default_rng(9), mosaic=0.5, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, cutout=(6, 9, 13))
    assert set(plan.n_place.tolist()) == {1, 4}
    rng = np.random.default_rng(10)
    targets = [{"boxes": np.stack([rng.uniform(0, w, 40), rng.uniform(0, h, 40), rng.uniform(1, w / 2, 40), rng.uniform(1, h / 2, 40)], axis=-1),
                "labels": rng.integers(0, 5, 40), "ids": rng.integers(0, 99, 40)} for (h, w) in sizes]
    first = cl.augment_batch(tensors, plan, targets, fill=FILL, hole_fill=HOLE_FILL)
    again = cl.augment_batch(tensors, plan, targets, fill=FILL, hole_fill=HOLE_FILL)
    assert torch.equal(first[0], again[0]) and all(torch.equal(first[1][k].view(torch.int64) if k == "boxes" else first[1][k],
                                                               again[1][k].view(torch.int64) if k == "boxes" else again[1][k]) for k in first[1])
    assert_same_bytes(first[0].cpu().numpy(), augment_ref.expected_canvas(frames, plan, FILL, HOLE_FILL))
    Gout = first[1]["boxes"].shape[1]
    assert Gout == 160 and int(first[1]["count"].sum()) > 40
    for n in range(len(plan)):
        canvas, t = cl.augment_batch(tensors, plan.single(n), targets, fill=FILL, hole_fill=HOLE_FILL)
        assert torch.equal(canvas[0], first[0][n])
        g = t["boxes"].shape[1]                  # a single canvas of one placement has Gout = Gmax
        assert int(t["count"][0]) == int(first[1]["count"][n])
        for k in ("boxes", "labels", "ids"):
            a, b = t[k][0], first[1][k][n]
            assert torch.equal(a.view(torch.int64).reshape(g, -1), b.view(torch.int64).reshape(Gout, -1)[:g])
            assert not b.view(torch.int64).reshape(Gout, -1)[g:].any()


# ----------------------------------------------------------------------------- (i): into the criteria
def test_train_augment_feeds_the_criteria():
    sizes = [(37, 53), (120, 200), (64, 48), (90, 160)]
    frames = [dev(f) for f in make_frames(sizes, 11)]
    rng = np.random.default_rng(12)
    listed = [{"boxes": np.stack([rng.uniform(0, 0.7 * w, 12), rng.uniform(0, 0.7 * h, 12), rng.uniform(0.1 * w, 0.3 * w, 12),
                                  rng.uniform(0.1 * h, 0.3 * h, 12)], axis=-1),
               "labels": rng.integers(0, 2, 12), "ids": rng.integers(0, 20, 12)} for (h, w) in sizes]
    N = len(sizes)
    g = torch.Generator().manual_seed(13)
    for with_ids in (False, True):
        augment = cl.TrainAugment(64, 64, seed=3, mosaic=1.0)
        given = listed if with_ids else [{k: v for k, v in d.items() if k != "ids"} for d in listed]
        canvas, targets = augment(frames, given)
        assert tuple(canvas.shape) == (N, 64, 64, 3) and set(augment.last_plan.n_place.tolist()) == {4}
        assert set(targets) == {"boxes", "labels", "count"} | ({"ids"} if with_ids else set())
        assert targets["boxes"].dtype == torch.float64 and targets["labels"].dtype == torch.int64 and targets["count"].dtype == torch.int32
        assert int(targets["count"].min()) >= 1
        outputs = {"heatmap": torch.randn((N, 2, 16, 16), generator=g).cuda().requires_grad_(),
                   "box_2d": (torch.rand((N, 4, 16, 16), generator=g) * 4 + 0.5).cuda().requires_grad_()}
        if with_ids:
            outputs["reid"] = torch.randn((N, 8, 16, 16), generator=g).cuda().requires_grad_()
            criterion = cl.TrackingLoss({}, cl.ReIDLoss(emb_dim=8, max_track_ids=20).cuda())
        else:
            criterion = cl.DetectionLoss()
        result = criterion(outputs, targets)
        total = result["total"]
        assert bool(torch.isfinite(total)) and float(total.detach()) > 0 and int(result["skipped"].sum()) == 0
        total.backward()
        for name, t in outputs.items():
            assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
