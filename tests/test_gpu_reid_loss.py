"""GPU: the re-ID loss (cnl_reid_loss_f64 / cnl_reid_loss_grad_f32, csrc/reid_loss.hip; loss.reid_loss, loss.reid_loss_grad, loss.ReIDLoss,
loss.TrackingLoss) against tests/reid_loss_ref.py, against the shipped forward's own central differences, against torch's own ops and through autograd.

Bounds.  Value and per_row: rtol 1e-8 against the restatement (the forward loss tests' own tolerance).  Gradients and the updated running statistics:
|gpu - fl32(ref)| <= one fp32 ulp of ref + C * max|ref| of that tensor, test_gpu_loss_grad.py's bound.  C: the restatement was run on the CPU with every
sum over rows taken in the opposite order, over all the cases below (measure_order_movement(), `python tests/test_gpu_reid_loss.py`): the largest movement
of any tensor was 3.5e-14 * max|ref| (the 900-row case; 2.0e-15 on the small cases; value: 3.4e-16 relative), below 1e-12 * max|ref|, so C = 1e-12, the
default.

Shapes: N = 3, H x W = 12 x 16, Gmax = 5, counts (5, 0, 3); D in 64 (two staged chunks of 32 features), 8, 20 (a partial chunk); K in 37 (a partial tile of
64 identities) and 2 * 64 + 3; two boxes in one cell, one box in cell (0, 0) (beside the padded rows with padded_rows), one in the last cell; both
padded_rows modes, both centre modes (box 3's centre truncs and rounds to different cells), training and eval.  big_case() runs every loop of the kernels more
than once: N = 3, Gmax = 300, counts (300, 40, 0), D in 96 and 160 (the 4- and 8-chunk forms of dz_kernel / dw2_kernel), K = 2 * 64 + 3; once more as
contiguous NCHW (the scatter's plane order with two staging passes).  seam_case(): one 16 x 40 image (2 x 2 tiles of 8 x 32), D = 8, Gmax = 8, a row on
each side of the tile seams (x = 31 | 32, y = 7 | 8) and in the four map corners: the edges of the scatter's staging predicate."""
import copy
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import reid_loss_ref as ref
import strided_io
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, loss

pytestmark = pytest.mark.gpu
STRIDE = 4
K_TILE = 64
C_ORDER = 1e-12
VALUE_RTOL = 1e-8                                            # of the float64 value and its per-row terms
N, H, W, GMAX = 3, 12, 16, 5
COUNTS = (5, 0, 3)
SHAPES = [(64, 37), (64, 2 * K_TILE + 3), (8, 37), (20, 37)]
MODES = list(itertools.product((False, True), ("trunc", "round"), (True, False)))      # padded_rows, center, training


def boxes_at(centres, sizes):
    c, s = np.asarray(centres, np.float64) * STRIDE, np.asarray(sizes, np.float64) * STRIDE
    return np.concatenate([c - s / 2, s], 1)


@functools.lru_cache(maxsize=None)
def case(D, K, seed=0):
    """-> (reid [N, D, H, W] f32, boxes [N, G, 4] (NaN beyond the count), ids [N, G] (-7 beyond the count), count, classifier dict of numpy fp32)"""
    rng = np.random.default_rng(100 * D + K + seed)
    boxes, ids = np.full((N, GMAX, 4), np.nan), np.full((N, GMAX), -7, np.int64)
    # image 0: two boxes in cell (5, 3), one in cell (0, 0), one in the last cell, one whose centre truncs to (9, 6) and rounds to (10, 7)
    boxes[0] = boxes_at([[5.3, 3.2], [5.4, 3.4], [0.3, 0.2], [W - 1 + 0.2, H - 1 + 0.3], [9.7, 6.6]], [[4, 3], [2, 5], [0.5, 0.4], [1, 1], [3, 3]])
    boxes[2, :3] = boxes_at([[2.2, 8.4], [12.6, 1.1], [7.49, 10.2]], [[3, 2], [5, 4], [2, 2]])
    ids[0] = rng.choice(K, 5, replace=False)
    ids[2, :3] = rng.choice(K, 3, replace=False)
    reid = rng.normal(0.0, 1.0, (N, D, H, W)).astype(np.float32)
    cls = dict(W1=rng.normal(0, 1 / np.sqrt(D), (D, D)), gamma=rng.uniform(0.5, 1.5, D), beta=rng.normal(0, 0.3, D), running_mean=rng.normal(0, 0.2, D),
               running_var=rng.uniform(0.5, 1.5, D), W2=rng.normal(0, 2 / np.sqrt(D), (K, D)), b2=rng.normal(0, 0.5, K))
    return reid, boxes, ids, np.array(COUNTS, np.int32), {k: v.astype(np.float32) for k, v in cls.items()}


BIG_N, BIG_G, BIG_COUNTS, BIG_K = 3, 300, (300, 40, 0), 2 * K_TILE + 3
BIG_D = (96, 160)                                            # 3 and 5 staged chunks: the 4- and 8-chunk forms of the two backward kernels
BIG_MODES = [(True, True), (False, True), (False, False)]    # padded_rows, training


@functools.lru_cache(maxsize=None)
def big_case(D):
    """Many rows: 340 live rows (11 row blocks of 32, two 256-slot passes of the counting and finishing loops, three 128-row tiles of the column sums, six
    64-row tiles of dW1), 900 stat rows with padded_rows; Gmax = 300 (two staging passes of the scatter, up to 8 rows in one cell); 4 rows without
    identity and 3 skipped ones.  -> as case()"""
    rng = np.random.default_rng(7000 + D)
    boxes, ids = np.full((BIG_N, BIG_G, 4), np.nan), np.full((BIG_N, BIG_G), -7, np.int64)
    for n, c in enumerate(BIG_COUNTS):
        centres = np.stack([rng.integers(0, W, c), rng.integers(0, H, c)], 1) + rng.uniform(0.05, 0.95, (c, 2))
        boxes[n, :c] = boxes_at(centres, rng.uniform(0.5, 6.0, (c, 2)))
        ids[n, :c] = rng.integers(0, BIG_K, c)
    ids[0, [5, 70, 257, 299]] = -1
    ids[0, 131], ids[1, 3] = BIG_K, BIG_K + 5
    boxes[0, 200, 0] = (W + 2.0) * STRIDE
    reid = rng.normal(0.0, 1.0, (BIG_N, D, H, W)).astype(np.float32)
    cls = dict(W1=rng.normal(0, 1 / np.sqrt(D), (D, D)), gamma=rng.uniform(0.5, 1.5, D), beta=rng.normal(0, 0.3, D), running_mean=rng.normal(0, 0.2, D),
               running_var=rng.uniform(0.5, 1.5, D), W2=rng.normal(0, 2 / np.sqrt(D), (BIG_K, D)), b2=rng.normal(0, 0.5, BIG_K))
    return reid, boxes, ids, np.array(BIG_COUNTS, np.int32), {k: v.astype(np.float32) for k, v in cls.items()}


@functools.lru_cache(maxsize=None)
def big_expected(D, padded, training):
    reid, boxes, ids, count, cls = big_case(D)
    kw = dict(training=training, stride=STRIDE, padded_rows=padded)
    return ref.reid_loss(reid, boxes, ids, count, cls, **kw), ref.reid_loss_grad(reid, boxes, ids, count, cls, **kw)


@functools.lru_cache(maxsize=None)
def expected(D, K, padded, center, training):
    reid, boxes, ids, count, cls = case(D, K)
    kw = dict(training=training, stride=STRIDE, center=center, padded_rows=padded)
    return ref.reid_loss(reid, boxes, ids, count, cls, **kw), ref.reid_loss_grad(reid, boxes, ids, count, cls, **kw)


def measure_order_movement():
    """The largest movement of any result, relative to the tensor's max|ref|, when the restatement sums over rows in the opposite order (CPU only)."""
    worst, worst_value = 0.0, 0.0
    small = [(case(D, K), dict(training=t, stride=STRIDE, center=c, padded_rows=p)) for (D, K), (p, c, t) in itertools.product(SHAPES, MODES)]
    big = [(big_case(D), dict(training=t, stride=STRIDE, padded_rows=p)) for D, (p, t) in itertools.product(BIG_D, BIG_MODES)]
    for (reid, boxes, ids, count, cls), kw in small + big:
        a, b = ref.reid_loss(reid, boxes, ids, count, cls, **kw), ref.reid_loss(reid, boxes, ids, count, cls, reverse=True, **kw)
        worst_value = max(worst_value, abs(a["reid"] - b["reid"]) / abs(a["reid"]))
        ga, gb = ref.reid_loss_grad(reid, boxes, ids, count, cls, **kw), ref.reid_loss_grad(reid, boxes, ids, count, cls, reverse=True, **kw)
        pairs = [(ga[k], gb[k]) for k in ref.GRADS] + [(a[k], b[k]) for k in ("running_mean64", "running_var64", "per_row")]
        for u, v in pairs:
            if np.abs(u).max() > 0:
                worst = max(worst, float(np.abs(u - v).max() / np.abs(u).max()))
    return worst, worst_value


def within(got, ref64, what):
    """|got - fl32(ref)| <= one fp32 ulp of ref + C_ORDER * max|ref|"""
    got = np.asarray(got, np.float32)
    ref32 = np.asarray(ref64, np.float64).astype(np.float32)
    assert got.shape == ref32.shape and np.isfinite(got).all(), what
    scale = float(np.abs(ref64).max(initial=0.0))
    tol = np.spacing(np.abs(ref32)).astype(np.float64) + C_ORDER * scale
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    worst = np.unravel_index(np.argmax(err - tol), err.shape) if err.size else ()
    print(what, "max|ref|", scale, "worst error", float(err.max(initial=0.0)), "elements off fl32(ref)", int(np.count_nonzero(got != ref32)), "of", got.size)
    assert (err <= tol).all(), (what, worst, float(got[worst]), float(ref32[worst]))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8),
                                                                       b.detach().contiguous().reshape(-1).view(torch.uint8))


def device_cls(cls):
    return {k: torch.from_numpy(v).cuda() for k, v in cls.items()}


def device_targets(boxes, ids, count):
    return {"boxes": torch.from_numpy(boxes).cuda(), "ids": torch.from_numpy(ids).cuda(), "count": torch.from_numpy(count).cuda()}


def run(D, K, padded, center, training, fmt=torch.channels_last, reid_t=None):
    reid, boxes, ids, count, cls = case(D, K)
    x = torch.from_numpy(reid).cuda().contiguous(memory_format=fmt) if reid_t is None else reid_t
    d = device_cls(cls)
    d["num_batches_tracked"] = torch.tensor(3, dtype=torch.int64, device="cuda")
    gts = device_targets(boxes, ids, count)
    kw = dict(training=training, stride=STRIDE, center=center, padded_rows=padded)
    grads = cl.reid_loss_grad(x, gts, d, **kw)
    value = cl.reid_loss(x, gts, d, **kw)
    return x, d, value, grads


def check_against_ref(value, d, grads, want, want_grad, training, what):
    np.testing.assert_allclose(float(value["reid"]), want["reid"], rtol=VALUE_RTOL, err_msg=what)
    np.testing.assert_allclose(value["per_row"].cpu().numpy(), want["per_row"], rtol=VALUE_RTOL, atol=0, err_msg=what)
    assert (int(value["num_rows"]), int(value["correct"]), int(value["skipped"])) == (want["num_rows"], want["correct"], want["skipped"]), what
    within(d["running_mean"].cpu().numpy(), want["running_mean64"], what + " running_mean")
    within(d["running_var"].cpu().numpy(), want["running_var64"], what + " running_var")
    assert int(d["num_batches_tracked"]) == 3 + (want["stepped"] if training else 0)
    for k in ref.GRADS:
        within(grads[k + "_grad"].cpu().numpy(), want_grad[k], f"{what} d {k}")
    g = grads["reid_grad"].cpu().numpy()
    unread = np.broadcast_to(~want_grad["read"][:, None], g.shape)
    assert (g[unread] == 0).all() and not np.signbit(g[unread]).any(), what      # exactly 0
    assert int(grads["skipped"]) == want["skipped"]


@pytest.mark.parametrize("padded,center,training", MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("D,K", SHAPES, ids=lambda v: str(v))
def test_value_and_gradients(D, K, padded, center, training):
    want, want_grad = expected(D, K, padded, center, training)
    assert want["num_rows"] == 8 and want["skipped"] == 0
    x, d, value, grads = run(D, K, padded, center, training)
    assert grads["reid_grad"].stride() == x.stride()
    check_against_ref(value, d, grads, want, want_grad, training, f"D{D} K{K} padded={padded} {center} training={training}")


@pytest.mark.parametrize("padded,training", BIG_MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("D", BIG_D)
def test_many_rows_and_wide_embeddings(D, padded, training):
    """Every loop of the kernels more than once (big_case), at the bounds of the small cases, and twice for identical bytes."""
    want, want_grad = big_expected(D, padded, training)
    assert want["num_rows"] == 333 and want["skipped"] == 3 and want_grad["read"].sum(axis=(1, 2)).tolist()[2] == (1 if padded and training else 0)
    reid, boxes, ids, count, cls = big_case(D)
    gts = device_targets(boxes, ids, count)
    kw = dict(training=training, stride=STRIDE, padded_rows=padded)
    runs = []
    for _ in range(2):
        x, d = torch.from_numpy(reid).cuda().contiguous(memory_format=torch.channels_last), device_cls(cls)
        d["num_batches_tracked"] = torch.tensor(3, dtype=torch.int64, device="cuda")
        grads = cl.reid_loss_grad(x, gts, d, **kw)
        value = cl.reid_loss(x, gts, d, **kw)
        runs.append([value["reid"], value["per_row"], d["running_mean"], d["running_var"]] + [grads[k + "_grad"] for k in ref.GRADS])
    check_against_ref(value, d, grads, want, want_grad, training, f"many rows D{D} padded={padded} training={training}")
    for a, b in zip(*runs):
        assert same_bits(a, b)


def test_plane_order_with_two_scatter_passes():
    """big_case(96) (Gmax = 300: two staging passes of the scatter) with the map and its gradient contiguous NCHW: the scatter walks the tile in plane
    order and restages both passes in every step.  The restatement's bound, and the bits of the channels-last run of the same inputs."""
    D, padded, training = 96, True, True
    want, want_grad = big_expected(D, padded, training)
    assert want["num_rows"] == 333 and want["skipped"] == 3
    reid, boxes, ids, count, cls = big_case(D)
    assert boxes.shape[1] == 300 > 256                        # more slots than one pass stages
    gts = device_targets(boxes, ids, count)
    kw = dict(training=training, stride=STRIDE, padded_rows=padded)
    runs = []
    for fmt in (torch.contiguous_format, torch.channels_last):
        x, d = torch.from_numpy(reid).cuda().contiguous(memory_format=fmt), device_cls(cls)
        d["num_batches_tracked"] = torch.tensor(3, dtype=torch.int64, device="cuda")
        grads = cl.reid_loss_grad(x, gts, d, **kw)
        value = cl.reid_loss(x, gts, d, **kw)
        assert grads["reid_grad"].stride() == x.stride()
        runs.append((value, d, grads))
    value, d, grads = runs[0]
    assert grads["reid_grad"].is_contiguous() and grads["reid_grad"].stride(3) == 1 and runs[1][2]["reid_grad"].stride(1) == 1
    check_against_ref(value, d, grads, want, want_grad, training, "plane order, two scatter passes")
    for k in ref.GRADS:
        assert same_bits(grads[k + "_grad"], runs[1][2][k + "_grad"]), k
    assert same_bits(value["per_row"], runs[1][0]["per_row"]) and same_bits(value["reid"], runs[1][0]["reid"])


SEAM_H, SEAM_W, SEAM_D, SEAM_K = 16, 40, 8, 37
SEAM_CELLS = [(31, 7), (32, 7), (31, 8), (32, 8), (0, 0), (SEAM_W - 1, 0), (0, SEAM_H - 1), (SEAM_W - 1, SEAM_H - 1)]      # the 8 x 32 tiles meet at x = 31 | 32, y = 7 | 8


@functools.lru_cache(maxsize=None)
def seam_case():
    """One image, Gmax = 8: a row in each of the four cells around the tiles' common corner and in the four corners of the map.  -> as case(), and the
    restatement's value and gradient"""
    rng = np.random.default_rng(31)
    boxes = boxes_at(np.asarray(SEAM_CELLS, np.float64) + 0.5, rng.uniform(1.0, 4.0, (len(SEAM_CELLS), 2)))[None]
    ids = rng.choice(SEAM_K, len(SEAM_CELLS), replace=False).astype(np.int64)[None]
    count = np.array([len(SEAM_CELLS)], np.int32)
    reid = rng.normal(0.0, 1.0, (1, SEAM_D, SEAM_H, SEAM_W)).astype(np.float32)
    D, K = SEAM_D, SEAM_K
    cls = dict(W1=rng.normal(0, 1 / np.sqrt(D), (D, D)), gamma=rng.uniform(0.5, 1.5, D), beta=rng.normal(0, 0.3, D), running_mean=rng.normal(0, 0.2, D),
               running_var=rng.uniform(0.5, 1.5, D), W2=rng.normal(0, 2 / np.sqrt(D), (K, D)), b2=rng.normal(0, 0.5, K))
    cls = {k: v.astype(np.float32) for k, v in cls.items()}
    kw = dict(training=True, stride=STRIDE)
    return (reid, boxes, ids, count, cls), ref.reid_loss(reid, boxes, ids, count, cls, **kw), ref.reid_loss_grad(reid, boxes, ids, count, cls, **kw)


@pytest.mark.parametrize("fmt", [torch.channels_last, torch.contiguous_format], ids=["nhwc", "nchw"])
def test_rows_on_both_sides_of_the_tile_seams_and_in_the_map_corners(fmt):
    """The scatter stages a row in the tile whose rectangle holds its cell (x0 <= x < x1, y0 <= y < y1): a row on either side of a seam, or in a corner
    of the map, belongs to exactly one tile, and every other element of the gradient is exactly +0."""
    (reid, boxes, ids, count, cls), want, want_grad = seam_case()
    assert want["num_rows"] == len(SEAM_CELLS) and want["skipped"] == 0
    assert sorted(zip(*np.nonzero(want_grad["read"][0])[::-1])) == sorted(SEAM_CELLS)
    assert {(x // 32, y // 8) for x, y in SEAM_CELLS} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for (x, y) in SEAM_CELLS:                                 # every planted row carries a gradient
        assert (want_grad["reid"][0, :, y, x] != 0).any(), (x, y)
    x, d = torch.from_numpy(reid).cuda().contiguous(memory_format=fmt), device_cls(cls)
    d["num_batches_tracked"] = torch.tensor(3, dtype=torch.int64, device="cuda")
    gts = device_targets(boxes, ids, count)
    grads = cl.reid_loss_grad(x, gts, d, training=True, stride=STRIDE)
    value = cl.reid_loss(x, gts, d, training=True, stride=STRIDE)
    check_against_ref(value, d, grads, want, want_grad, True, "tile seams and map corners")
    g = grads["reid_grad"].cpu().numpy()
    assert np.array_equal((g != 0).any(axis=1), want_grad["read"])


def test_rules_skipped_ignored_and_cells():
    D, K = 8, 37
    reid, boxes, ids, count, cls = case(D, K)
    boxes, ids = boxes.copy(), ids.copy()
    ids[0, 1] = -1                                            # without identity: dropped silently
    ids[0, 4] = K                                             # outside the classifier: skipped
    boxes[2, 0] = boxes_at([[W + 0.5, 3.0]], [[2, 2]])[0]     # cell outside the map: skipped
    boxes[2, 1, 2] = -1.0                                     # negative width: skipped
    gts = device_targets(boxes, ids, count)
    for center, padded in (("trunc", False), ("round", True)):
        kw = dict(training=True, stride=STRIDE, center=center, padded_rows=padded)
        want, want_grad = ref.reid_loss(reid, boxes, ids, count, cls, **kw), ref.reid_loss_grad(reid, boxes, ids, count, cls, **kw)
        assert want["num_rows"] == 4 and want["skipped"] == 3
        x, d = torch.from_numpy(reid).cuda(), device_cls(cls)
        d["num_batches_tracked"] = torch.tensor(3, dtype=torch.int64, device="cuda")
        grads = cl.reid_loss_grad(x, gts, d, **kw)
        value = cl.reid_loss(x, gts, d, **kw)
        check_against_ref(value, d, grads, want, want_grad, True, f"rules {center}")
    # ignore_index is a setting: with -5 the row of id -1 is a skipped one
    assert int(cl.reid_loss(torch.from_numpy(reid).cuda(), gts, device_cls(cls), stride=STRIDE, ignore_index=-5)["skipped"]) == 4


def test_layouts_same_bits_and_guards():
    D, K = 64, 2 * K_TILE + 3
    reid = case(D, K)[0]
    for padded, training in ((True, True), (False, False)):
        outs = []
        views = [strided_io.StridedView(torch.from_numpy(reid), layout, poison="nan", device="cuda") for layout in ("nchw", "nhwc", "nhwc_wide")]
        for v in views:
            x, d, value, grads = run(D, K, padded, "trunc", training, reid_t=v.view)
            assert v.unchanged(), v.layout
            outs.append([value["reid"], value["per_row"], d["running_mean"], d["running_var"]] + [grads[k + "_grad"] for k in ref.GRADS])
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert same_bits(a, b)


def test_gradient_into_a_guarded_slice():
    """The map's gradient written into a 64-channel slice of a wider, sentinel-filled buffer: every element of the slice written, nothing else."""
    D, K = 64, 37
    reid, boxes, ids, count, cls = case(D, K)
    want_grad = expected(D, K, True, "trunc", True)[1]
    x = strided_io.StridedView(torch.from_numpy(reid), "nhwc_wide", poison="nan", device="cuda")
    out = strided_io.Guarded((N, H, W), D, ld=D + 12, off=4, device="cuda", name="d reid")
    g = out.view.permute(0, 3, 1, 2)                          # logical [N, D, H, W]
    d, gts = device_cls(cls), device_targets(boxes, ids, count)
    t = {k: d[k] for k in loss.REID_KEYS}
    params = loss.reid_params(True, STRIDE, "trunc", True, -1)
    lib = _lib.load()
    nbytes = lib.cnl_reid_loss_grad_workspace_bytes(N, GMAX, D)
    ws = strided_io.GuardedBytes(nbytes, align=16, device="cuda", name="workspace")
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    others = [torch.empty_like(t[k]) for k in ref.GRADS[1:]]
    common = loss._reid_common(x.view, (N, D, H, W), K, t, (gts["boxes"], gts["ids"], gts["count"]), params)
    _lib.check(lib.cnl_reid_loss_grad_f32(*common, None, g.data_ptr(), *g.stride(), *(o.data_ptr() for o in others), skipped.data_ptr(), ws.ptr, nbytes,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "cnl_reid_loss_grad_f32")
    torch.cuda.synchronize()
    ok, msg = out.verdict()
    assert ok, msg
    assert out.unwritten() == 0
    ok, msg = ws.verdict()
    assert ok, msg
    assert x.unchanged()
    within(g.cpu().numpy(), want_grad["reid"], "guarded d reid")
    for k, o in zip(ref.GRADS[1:], others):
        within(o.cpu().numpy(), want_grad[k], "guarded d " + k)


def test_two_runs_identical_bytes():
    a, b = run(64, 2 * K_TILE + 3, True, "trunc", True), run(64, 2 * K_TILE + 3, True, "trunc", True)
    for u, v in ((a[2]["reid"], b[2]["reid"]), (a[2]["per_row"], b[2]["per_row"]), (a[1]["running_var"], b[1]["running_var"])):
        assert same_bits(u, v)
    for k in ref.GRADS:
        assert same_bits(a[3][k + "_grad"], b[3][k + "_grad"]), k


def test_eval_row_does_not_depend_on_the_batch():
    D, K = 20, 37
    reid, boxes, ids, count, cls = case(D, K)
    d = device_cls(cls)
    whole = cl.reid_loss(torch.from_numpy(reid).cuda(), device_targets(boxes, ids, count), d, training=False, stride=STRIDE)["per_row"]
    for n in (0, 2):
        alone = cl.reid_loss(torch.from_numpy(reid[n:n + 1]).cuda(), device_targets(boxes[n:n + 1], ids[n:n + 1], count[n:n + 1]), d, training=False,
                             stride=STRIDE)["per_row"]
        assert same_bits(alone[0], whole[n])


def test_large_logits_stay_finite():
    D, K = 20, 2 * K_TILE + 3
    reid, boxes, ids, count, cls = case(D, K)
    cls = {k: v.copy() for k, v in cls.items()}
    rng = np.random.default_rng(5)
    cls["b2"] = (rng.choice([-800.0, 800.0], K) + rng.normal(0, 1, K)).astype(np.float32)
    cls["W2"] = (cls["W2"] * 20).astype(np.float32)
    for training in (True, False):
        want = ref.reid_loss(reid, boxes, ids, count, cls, training=training, stride=STRIDE)
        got = cl.reid_loss(torch.from_numpy(reid).cuda(), device_targets(boxes, ids, count), device_cls(cls), training=training, stride=STRIDE)
        assert np.isfinite(want["reid"]) and want["reid"] > 100
        assert torch.isfinite(got["reid"]) and torch.isfinite(got["per_row"]).all()
        np.testing.assert_allclose(float(got["reid"]), want["reid"], rtol=1e-8)
        np.testing.assert_allclose(got["per_row"].cpu().numpy(), want["per_row"], rtol=1e-8)
        assert int(got["correct"]) == want["correct"]


@pytest.mark.parametrize("training,padded", [(True, True), (True, False), (False, False)])
def test_central_differences_of_the_shipped_forward(training, padded):
    """<grad, d> against (f(x + h d) - f(x - h d)) / 2h of reid_loss itself, d a random direction over the map and every parameter; inputs are multiples
    of 2^-12 and h d of 2^-11, so x +- h d are exact in fp32.  The training run differentiates through the batch statistics."""
    D, K = 20, 37
    reid, boxes, ids, count, cls = case(D, K)
    q = lambda a: (np.round(a * 4096) / 4096).astype(np.float32)
    rng = np.random.default_rng(11)
    x0 = {"reid": q(reid), **{k: q(cls[k]) for k in ("W1", "gamma", "beta", "W2", "b2")}}
    fixed = {k: q(cls[k]) for k in ("running_mean", "running_var")}
    direction = {k: rng.choice([-1.0, -0.5, 0.5, 1.0], v.shape).astype(np.float32) for k, v in x0.items()}
    h = 2.0 ** -10
    gts = device_targets(boxes, ids, count)
    kw = dict(training=training, stride=STRIDE, padded_rows=padded)

    def f(sign):
        v = {k: torch.from_numpy(x0[k] + np.float32(sign * h) * direction[k]).cuda() for k in x0}
        d = {**{k: v[k] for k in v if k != "reid"}, **{k: torch.from_numpy(a).cuda() for k, a in fixed.items()}}
        return float(cl.reid_loss(v["reid"], gts, d, update_stats=False, **kw)["reid"])

    d0 = {**{k: torch.from_numpy(x0[k]).cuda() for k in x0 if k != "reid"}, **{k: torch.from_numpy(a).cuda() for k, a in fixed.items()}}
    grads = cl.reid_loss_grad(torch.from_numpy(x0["reid"]).cuda(), gts, d0, **kw)
    dot = sum(float((grads[k + "_grad"].double().cpu() * torch.from_numpy(direction[k]).double()).sum()) for k in x0)
    numeric = (f(+1) - f(-1)) / (2 * h)
    print("central difference", numeric, "<grad, d>", dot)
    np.testing.assert_allclose(dot, numeric, rtol=1e-4)


def torch_reference(module, reid, boxes, ids, count, training):
    """The same gathered rows through a float64 copy of the module's classifier and F.cross_entropy, on the device."""
    seq = copy.deepcopy(module.classifier).double()
    seq.train(training)
    state, x, y, _ = ref.rows_of(boxes, ids, count, H, W, module.max_track_ids, STRIDE)
    n, g = np.nonzero(state == 2)
    x64 = reid.detach().double().requires_grad_(True)
    rows = x64[torch.from_numpy(n).cuda(), :, torch.from_numpy(y[n, g]).cuda(), torch.from_numpy(x[n, g]).cuda()]
    logits = seq(rows)
    value = torch.nn.functional.cross_entropy(logits, torch.from_numpy(ids[n, g]).cuda(), reduction="sum") / (len(n) + 1e-8)
    value.backward()
    return value, x64.grad, seq


@pytest.mark.parametrize("training", [True, False])
def test_module_against_torch_ops(training):
    D, K = 64, 37
    reid, boxes, ids, count, _ = case(D, K)
    torch.manual_seed(3)
    module = cl.ReIDLoss(D, K, stride=STRIDE).cuda()
    with torch.no_grad():
        module.classifier[1].running_mean.normal_(0, 0.2)
        module.classifier[1].running_var.uniform_(0.5, 1.5)
        module.classifier[1].weight.uniform_(0.5, 1.5)
        module.classifier[1].bias.normal_(0, 0.3)
    module.train(training)
    x = torch.from_numpy(reid).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    want, want_x, seq = torch_reference(module, x, boxes, ids, count, training)
    out = module({"reid": x}, device_targets(boxes, ids, count))
    assert out["reid"].grad_fn is not None and out["reid"].dtype == torch.float64
    out["reid"].backward()
    close = lambda a, b, what: torch.testing.assert_close(a.double(), b, rtol=1e-6, atol=1e-12 * float(b.abs().max()), msg=lambda m: f"{what}: {m}")
    close(out["reid"].detach(), want.detach(), "value")
    close(x.grad, want_x, "d reid")
    for (name, p), (_, p64) in zip(module.classifier.named_parameters(), seq.named_parameters()):
        close(p.grad, p64.grad, "d " + name)
    bn, bn64 = module.classifier[1], seq[1]
    close(bn.running_mean, bn64.running_mean, "running_mean")
    close(bn.running_var, bn64.running_var, "running_var")
    assert int(bn.num_batches_tracked) == int(bn64.num_batches_tracked) == (1 if training else 0)


def test_tracking_loss_reaches_a_conv_head():
    D, K, C = 8, 37, 3
    reid, boxes, ids, count, _ = case(D, K)
    rng = np.random.default_rng(2)
    labels = rng.integers(0, C, ids.shape).astype(np.int64)
    torch.manual_seed(4)
    head = torch.nn.Conv2d(6, C + 4 + D, 3, padding=1).cuda()
    feat = torch.randn(N, 6, H, W, device="cuda")
    reid_module = cl.ReIDLoss(D, K, loss_weight=0.7, stride=STRIDE).cuda()
    criterion = cl.TrackingLoss(dict(stride=STRIDE, box_loss_weight=2.0), reid_module)
    targets = {"boxes": torch.from_numpy(boxes).cuda(), "labels": torch.from_numpy(labels).cuda(), "ids": torch.from_numpy(ids).cuda(),
               "count": torch.from_numpy(count).cuda()}

    def outputs():
        y = head(feat)
        maps = {"heatmap": y[:, :C], "box_2d": y[:, C:C + 4], "reid": y[:, C + 4:]}
        for m in maps.values():
            m.retain_grad()
        return maps

    def grads_of(total, maps):
        head.zero_grad()
        reid_module.zero_grad()
        total.backward()
        return [None if maps[k].grad is None else maps[k].grad.clone() for k in ("heatmap", "box_2d", "reid")], [p.grad.clone() for p in head.parameters()], \
            [p.grad.clone() if p.grad is not None else None for p in reid_module.parameters()]

    maps = outputs()
    res = criterion(maps, targets)
    both = grads_of(res["total"], maps)
    maps = outputs()
    det = cl.DetectionLoss(stride=STRIDE, box_loss_weight=2.0)(maps, targets)
    for k in ("heatmap", "box_2d"):
        assert same_bits(res[k], det[k])
    det_only = grads_of(det["total"], maps)
    maps = outputs()
    rid = reid_module(maps, targets)
    reid_only = grads_of(0.7 * rid["reid"], maps)
    assert torch.equal(res["reid"].detach(), rid["reid"].detach())
    torch.testing.assert_close(res["total"].detach(), det["total"].detach() + 0.7 * rid["reid"].detach(), rtol=1e-15, atol=0)
    for i in (0, 1):
        assert torch.equal(both[0][i], det_only[0][i])        # the maps' gradients: the same bits
    assert torch.equal(both[0][2], reid_only[0][2]) and det_only[0][2] is None and reid_only[0][0] is None
    for a, b, c in zip(both[1], det_only[1], reid_only[1]):
        assert a.abs().max() > 0
        torch.testing.assert_close(a, b + c, rtol=1e-5, atol=1e-6 * float(a.abs().max()))
    for a, c in zip(both[2], reid_only[2]):
        assert a is not None and torch.equal(a, c)
    skip = criterion(outputs(), targets, ignore_reid=True)
    assert torch.equal(skip["total"].detach(), det["total"].detach()) and float(skip["reid"]) == 0.0
    tuple_form = criterion(outputs(), (targets["boxes"], targets["labels"], targets["count"], targets["ids"]))
    assert torch.equal(tuple_form["total"].detach(), res["total"].detach())


def test_fewer_than_two_stat_rows():
    D, K = 8, 37
    reid, boxes, ids, count, cls = case(D, K)
    one = np.array([0, 0, 1], np.int32)
    x, gts = torch.from_numpy(reid).cuda(), device_targets(boxes, ids, one)
    d = device_cls(cls)
    d["num_batches_tracked"] = torch.tensor(3, dtype=torch.int64, device="cuda")
    before = {k: v.clone() for k, v in d.items()}
    value = cl.reid_loss(x, gts, d, training=True, stride=STRIDE)
    grads = cl.reid_loss_grad(x, gts, d, training=True, stride=STRIDE)
    assert float(value["reid"]) == 0.0 and not value["per_row"].any() and int(value["num_rows"]) == 1
    for k in ref.GRADS:
        assert not grads[k + "_grad"].any(), k
    for k in d:
        assert torch.equal(d[k], before[k]), k
    # one row in eval mode is an ordinary call
    want, want_grad = ref.reid_loss(reid, boxes, ids, one, cls, training=False, stride=STRIDE), ref.reid_loss_grad(reid, boxes, ids, one, cls, training=False, stride=STRIDE)
    value = cl.reid_loss(x, gts, d, training=False, stride=STRIDE)
    grads = cl.reid_loss_grad(x, gts, d, training=False, stride=STRIDE)
    assert want["num_rows"] == 1 and want["reid"] > 0
    check_against_ref(value, d, grads, want, want_grad, False, "one row, eval")


def test_host_list_targets_and_no_grad_module():
    D, K = 8, 37
    reid, boxes, ids, count, cls = case(D, K)
    host = [{"boxes": boxes[n, :c], "ids": ids[n, :c]} for n, c in enumerate(count)]
    x = torch.from_numpy(reid).cuda()
    a = cl.reid_loss(x, host, device_cls(cls), stride=STRIDE)
    b = cl.reid_loss(x, device_targets(boxes, ids, count), device_cls(cls), stride=STRIDE)
    assert torch.equal(a["reid"], b["reid"]) and torch.equal(a["per_row"], b["per_row"])
    module = cl.ReIDLoss(D, K, stride=STRIDE).cuda()
    with torch.no_grad():
        out = module({"reid": x}, host)
    assert out["reid"].grad_fn is None and int(module.classifier[1].num_batches_tracked) == 1


if __name__ == "__main__":
    print("movement with the row order reversed: %.3e * max|ref| (value: %.3e relative)" % measure_order_movement())
