"""GPU: the gradient of the detection loss (cnl_detection_loss_grad_f32, csrc/det_loss.hip; loss.detection_loss_grad, loss.DetectionLoss) against
tests/loss_grad_ref.py, against the shipped forward's own central differences, and through torch's autograd.

Bound.  |gpu - fl32(ref)| <= one fp32 ulp of ref + 1e-12 * max|ref| of that tensor: the device and numpy differ by a few float64 ulps in exp / log1p /
atan, on terms no larger than (|x| + 2) times the element's scale with |x| <= 10, and one rounding to fp32 follows.  With box_log the device's and
the host's fp32 exp may differ by an ulp or two of the box size: 1e-5 * max|ref| on the box gradient, the forward tests' own allowance.  Pixels no
sample touches are exactly 0.

Shapes are the smallest that reach each path: H x W in 1x1, 3x5, 16x20, 33x70 (tiles are 8 x 32: 33x70 has 5 x 3 tiles with partial last tiles both
ways), C in 1, 2, 3, 81, boxes per image 0, 1, 9 and PASS_SLOTS + 44 (two staging passes); W * C a multiple of 4 (the 16-byte path of packed
channels-last maps: edges, c81, two_pass, iou, log) and not (small, tiles)."""
import ctypes
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

import loss_grad_ref
import loss_ref
import strided_io
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "grad_loss_*.npz")))
GOLDEN_NAMES = [os.path.basename(p)[10:-4] for p in GOLDEN]
PASS_SLOTS = 256
TILE_H, TILE_W = 8, 32
STRIDE = 4
LOG_RTOL = 1e-5


def boxes_at(centres, sizes):
    """x y w h in input pixels with the given centres and sizes in map pixels."""
    c, s = np.asarray(centres, np.float64) * STRIDE, np.asarray(sizes, np.float64) * STRIDE
    return np.concatenate([c - s / 2, s], 1)


def random_targets(rng, m, C, H, W, max_size=10.0, min_size=0.5):
    centres = np.stack([rng.integers(0, W, m), rng.integers(0, H, m)], 1) + rng.uniform(-0.4, 0.4, (m, 2))
    return boxes_at(centres, rng.uniform(min_size, max_size, (m, 2))), rng.integers(0, C, m).astype(np.int64)


def pad(targets):
    """[(boxes, labels)] -> (boxes [N,G,4] with NaN beyond the count, labels, count)"""
    G = max([1] + [len(lab) for _, lab in targets])
    boxes, labels = np.full((len(targets), G, 4), np.nan), np.full((len(targets), G), -7, np.int64)
    for n, (b, lab) in enumerate(targets):
        boxes[n, :len(lab)], labels[n, :len(lab)] = b, lab
    return boxes, labels, np.array([len(lab) for _, lab in targets], np.int32)


CASES = {
    # name: (seed, (N, C, H, W), boxes per image, settings)
    "pixel": (1, (1, 1, 1, 1), [1], dict(heatmap_target="fixed", heatmap_target_params={"r": 0.0}, box_loss="l1")),
    "small": (2, (2, 2, 3, 5), [1, 0], dict(heatmap_target="ttfnet", heatmap_target_params={"alpha": 3.0}, heatmap_loss="quality", box_loss="l1")),
    "edges": (3, (2, 3, 16, 20), [9, 1], dict(box_loss="giou", box_loss_weight=5.0)),
    "c81": (5, (2, 81, 16, 20), [9, 0], dict(heatmap_loss="quality", box_loss="smooth_l1", box_multiplier=16.0, heatmap_loss_weight=0.5)),
    "two_pass": (6, (1, 2, 16, 20), [PASS_SLOTS + 44], dict(box_loss="diou", heatmap_target="fixed")),
    "tiles": (7, (2, 3, 33, 70), [9, 9], dict(box_loss="ciou", heatmap_target="ttfnet")),
    "iou": (9, (1, 2, 33, 70), [9], dict(box_loss="iou")),
    "log": (8, (1, 1, 16, 20), [9], dict(box_log=True, box_loss="l1")),
    "log_giou": (10, (1, 3, 16, 20), [9], dict(box_log=True, box_loss="giou", heatmap_loss="quality")),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (heat [N,C,H,W] f32, box [N,4,H,W] f32, [(boxes, labels)], settings)"""
    if name.startswith("golden:"):
        z = np.load(GOLDEN[GOLDEN_NAMES.index(name[7:])])
        assert int(z["stride"]) == STRIDE
        return z["heat"], z["box"], [(z["boxes"][n, :c], z["labels"][n, :c]) for n, c in enumerate(z["count"])], json.loads(str(z["settings"]))
    seed, (N, C, H, W), counts, settings = CASES[name]
    rng = np.random.default_rng(seed)
    targets = []
    for n in range(N):
        b, lab = random_targets(rng, counts[n], C, H, W, *((18.0, 14.0) if name.startswith("log") else ()))
        if name == "small" and n == 0:
            b, lab = boxes_at([[2.0, 1.0]], [[4.0, 3.0]]), np.array([1])
        if name == "edges" and n == 0:                       # centres at 0, W - 1, ON W and ON H; overlapping boxes of one class and of two
            b = boxes_at([[0, 0], [W - 1, 5], [W, 9], [7, H], [W, H], [6, 6], [8, 7], [7, 6], [12.5, 3.5]],
                         [[4, 4], [6, 5], [6, 6], [5, 6], [4, 4], [9, 8], [9, 9], [8, 8], [3, 2]])
            lab = np.array([0, 1, 2, 0, 1, 1, 1, 2, 0])
        if name == "two_pass":                               # all of them reach the first tile
            b[:, :2] = np.stack([rng.integers(0, 20, len(b)), rng.integers(0, 8, len(b))], 1) * STRIDE - b[:, 2:] / 2
        targets.append((b, lab.astype(np.int64)))
    heat = rng.normal(-2.0, 2.0, (N, C, H, W)).astype(np.float32)
    if settings.get("box_log"):
        box = rng.uniform(-1.0, 1.2, (N, 4, H, W)).astype(np.float32)
    else:
        box = (rng.uniform(-0.5, 6.0, (N, 4, H, W)) / settings.get("box_multiplier", 1.0)).astype(np.float32)
    return heat, box, targets, settings


@functools.lru_cache(maxsize=None)
def expected(name, heatmap_scale=1.0, box_scale=1.0):
    heat, box, targets, settings = case(name)
    return loss_grad_ref.detection_loss_grad(heat, box, targets, stride=STRIDE, heatmap_scale=heatmap_scale, box_scale=box_scale, **settings)


def device_targets(padded):
    return tuple(torch.from_numpy(a).cuda() for a in padded)


def within(got, ref64, what, rtol=0.0):
    """|got - fl32(ref)| <= one fp32 ulp of ref + (1e-12 + rtol) * max|ref|"""
    got = np.asarray(got, np.float32)
    with np.errstate(over="ignore", under="ignore"):
        ref = np.asarray(ref64, np.float64).astype(np.float32)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    scale = float(np.abs(ref64).max(initial=0.0))
    tol = np.spacing(np.abs(ref)).astype(np.float64) + (1e-12 + rtol) * scale
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    worst = np.unravel_index(np.argmax(err - tol), err.shape) if err.size else ()
    print(what, "max|ref|", scale, "worst error", float(err.max(initial=0.0)), "elements off by one fp32 ulp", int(np.count_nonzero(got != ref)), "of", got.size)
    assert (err <= tol).all(), (what, worst, float(got[worst]), float(ref[worst]))


def check(out_heat, out_box, skipped, want, settings, what):
    if out_heat is not None:
        within(out_heat, want["heatmap_grad64"], what + " heatmap")
    if out_box is not None:
        within(out_box, want["box_2d_grad64"], what + " box_2d", LOG_RTOL if settings.get("box_log") else 0.0)
        untouched = np.broadcast_to(~want["touched"][:, None], np.shape(out_box))
        assert (np.asarray(out_box)[untouched] == 0).all() and not np.signbit(np.asarray(out_box)[untouched]).any(), what      # exactly 0
    assert int(skipped) == want["skipped"]


def api(name, channels_last=True, **kw):
    heat, box, targets, settings = case(name)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    h = torch.from_numpy(heat).cuda().contiguous(memory_format=fmt)
    b = torch.from_numpy(box).cuda().contiguous(memory_format=fmt)
    return h, b, cl.detection_loss_grad(h, b, device_targets(pad(targets)), stride=STRIDE, **settings, **kw)


# ----------------------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("name", list(CASES))
def test_gradient_against_the_restatement(name):
    want = expected(name)
    h, b, out = api(name)
    assert out["heatmap_grad"].dtype == torch.float32 and out["heatmap_grad"].stride() == h.stride() and out["box_2d_grad"].stride() == b.stride()
    assert out["skipped"].dim() == 0 and out["skipped"].dtype == torch.int32
    check(out["heatmap_grad"].cpu().numpy(), out["box_2d_grad"].cpu().numpy(), out["skipped"], want, case(name)[3], name)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_gradient_on_the_goldens_inputs(name):
    """The reference's fixtures (contiguous NCHW, as they are stored), the planted ties among them."""
    want = expected("golden:" + name)
    h, b, out = api("golden:" + name, channels_last=False)
    assert out["heatmap_grad"].is_contiguous() and out["box_2d_grad"].is_contiguous()
    check(out["heatmap_grad"].cpu().numpy(), out["box_2d_grad"].cpu().numpy(), out["skipped"], want, case("golden:" + name)[3], name)
    if name.startswith("ties"):
        z = np.load(GOLDEN[GOLDEN_NAMES.index(name)])         # and the reference's own autograd, at the host test's allowance plus the rounding to fp32
        for got, ref in ((out["heatmap_grad"], z["d_heatmap_d_heat"]), (out["box_2d_grad"], z["d_box_d_box"])):
            assert np.abs(got.cpu().numpy() - ref).max() <= (4 * float(z["tol64"]) + 2.0 ** -23) * np.abs(ref).max()


def test_two_passes_are_needed():
    recs = loss_ref.records(*case("two_pass")[2][0], 2, 16, 20, STRIDE, "fixed", None)
    near = [r for r in recs if r["state"] and r["cx"] - 1 < TILE_W and r["cy"] - 1 < TILE_H]
    assert len(recs) > PASS_SLOTS and len(near) > PASS_SLOTS and any(r in near for r in recs[PASS_SLOTS:])
    assert expected("two_pass")["contributions"].max() >= 5


def test_log_inputs_stay_away_from_the_ties():
    """The premise of LOG_RTOL: the device's and the host's fp32 exp may move a decoded corner (below 128 input pixels here) by an ulp or two, 2e-5 of
    a pixel; every sample of the box_log cases is farther than 1e-3 of a pixel from every tie, so no branch of the rule changes sides, and a smooth
    loss's derivative moves by that over the box size, 1e-6."""
    for name in ("log", "log_giou"):
        heat, box, targets, settings = case(name)
        assert loss_grad_ref.tie_distance(box, targets, heat.shape[1], **settings) > 1e-3


# ----------------------------------------------------------------------------- seams, corners, stacked boxes
def boxes_inputs(shape, boxes, labels, settings, seed=11):
    """-> (heat, box, targets, the restatement's result) of boxes given for the first image"""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    heat = rng.normal(-2.0, 2.0, shape).astype(np.float32)
    box = rng.uniform(-0.5, 6.0, (N, 4, H, W)).astype(np.float32)
    targets = [(np.asarray(boxes, np.float64), np.asarray(labels, np.int64))] + [(np.zeros((0, 4)), np.zeros((0,), np.int64))] * (N - 1)
    return heat, box, targets, loss_grad_ref.detection_loss_grad(heat, box, targets, stride=STRIDE, **settings)


def run_boxes(heat, box, targets, want, settings):
    h = torch.from_numpy(heat).cuda().contiguous(memory_format=torch.channels_last)
    b = torch.from_numpy(box).cuda().contiguous(memory_format=torch.channels_last)
    out = cl.detection_loss_grad(h, b, device_targets(pad(targets)), stride=STRIDE, **settings)
    check(out["heatmap_grad"].cpu().numpy(), out["box_2d_grad"].cpu().numpy(), out["skipped"], want, settings, "boxes")
    return out


SEAM_H, SEAM_W = 33, 70
SEAM_CENTRES = [(x, y) for x in (31, 32, 63, 64) for y in (7, 8, 31, 32)] + [(0, 0), (SEAM_W - 1, SEAM_H - 1), (SEAM_W, 20), (40, SEAM_H), (SEAM_W, SEAM_H)]
SEAM_SETTINGS = dict(heatmap_target="fixed", heatmap_target_params={"r": 0.0}, box_loss="giou")


@functools.lru_cache(maxsize=None)
def seam_inputs():
    return boxes_inputs((1, 2, SEAM_H, SEAM_W), boxes_at(SEAM_CENTRES, [[5.0, 4.0]] * len(SEAM_CENTRES)), [i % 2 for i in range(len(SEAM_CENTRES))],
                        SEAM_SETTINGS)


def test_radius_0_boxes_on_both_sides_of_every_tile_seam_and_at_the_corners():
    """A radius-0 box renders one pixel and samples nine: staging by the rendered window would lose the samples across a seam."""
    H, W = SEAM_H, SEAM_W
    heat, box, targets, want = seam_inputs()
    samples = [(x, y) for (cx, cy) in SEAM_CENTRES for x in range(max(cx - 1, 0), min(cx + 1, W - 1) + 1) for y in range(max(cy - 1, 0), min(cy + 1, H - 1) + 1)]
    assert want["num_dets"] == len(SEAM_CENTRES) and want["num_boxes"] == len(samples) and want["skipped"] == 0
    assert [r["rx"] for r in loss_ref.records(*targets[0], 2, H, W, STRIDE, "fixed", 0.0)] == [0] * len(SEAM_CENTRES)
    for (x, y) in samples:                                   # every sample carries a gradient, across the seams too ...
        assert want["touched"][0, y, x] and (want["box_2d_grad"][0, :, y, x] != 0).any(), (x, y)
    assert {x // TILE_W for x, _ in samples} == {0, 1, 2} and {y // TILE_H for _, y in samples} == {0, 1, 2, 3, 4}
    out = run_boxes(heat, box, targets, want, SEAM_SETTINGS)
    got = out["box_2d_grad"].cpu().numpy()
    assert np.array_equal((got != 0).any(axis=1), (want["box_2d_grad"] != 0).any(axis=1))      # ... and the device gives every one of them, and no other pixel


STACK_CENTRES = [(10, 9), (10, 9), (10, 9), (11, 9), (11, 10), (9, 8), (10, 10), (10, 9), (31, 7), (32, 8), (32, 8), (31, 8), (33, 7), (32, 7)]
STACK_LABELS = [0, 0, 1, 2, 0, 1, 1, 2, 0, 0, 1, 2, 2, 0]


@functools.lru_cache(maxsize=None)
def stack_inputs(kind):
    sizes = [[3.0 + 0.5 * i, 6.0 - 0.25 * i] for i in range(len(STACK_CENTRES))]
    settings = dict(box_loss=kind, heatmap_target="ttfnet")
    return boxes_inputs((2, 3, 33, 70), boxes_at(STACK_CENTRES, sizes), STACK_LABELS, settings) + (settings,)


@pytest.mark.parametrize("kind", ["giou", "smooth_l1"])
def test_stacked_boxes_add_up_in_slot_order(kind):
    heat, box, targets, want, settings = stack_inputs(kind)
    assert want["contributions"].max() >= 8 and np.count_nonzero(want["contributions"] >= 5) >= 6
    run_boxes(heat, box, targets, want, settings)


# ----------------------------------------------------------------------------- the C ABI: layouts, guarded outputs, exact workspace
OUT_LAYOUTS = ("nhwc", "nchw", "every_other_channel")


def guarded_map(shape, layout, align, name):
    """An fp32 [N, C, H, W] output of the layout inside a byte-guarded buffer of NaN bytes -> (GuardedBytes, strides in elements)"""
    N, C, H, W = shape
    if layout == "nhwc":
        strides, floats, mask = (H * W * C, 1, W * C, C), N * H * W * C, None
    elif layout == "nchw":
        strides, floats, mask = (C * H * W, H * W, W, 1), N * C * H * W, None
    else:                                                     # channels 0, 2, 4 ... of 2 C channels, NHWC storage
        strides, floats = (H * W * 2 * C, 2, W * 2 * C, 2 * C), N * H * W * 2 * C
        mask = (torch.arange(floats) % 2 == 0).repeat_interleave(4)
    return strided_io.GuardedBytes(floats * 4, align=align, device="cuda", sentinel=0xFF, mask=mask, name=name), strides


def launch(name, in_layout="nhwc", out_layouts=("nhwc", "nhwc"), wanted=(True, True), scales=None, align=4):
    """One raw call.  -> (heatmap gradient or None, box gradient or None, skipped), numpy"""
    heat, box, targets, settings = case(name)
    N, C, H, W = heat.shape
    lib = _lib.load()
    hv = strided_io.StridedView(torch.from_numpy(heat), in_layout, poison="nan", device="cuda", name="heat")
    bv = strided_io.StridedView(torch.from_numpy(box), in_layout, poison="inf", device="cuda", name="box")
    gts = device_targets(pad(targets))
    G = gts[0].shape[1]
    nbytes = lib.cnl_detection_loss_grad_workspace_bytes(N, G, H, W)
    assert nbytes == N * G * 32 + 16
    ws = strided_io.GuardedBytes(nbytes, align=16, device="cuda", name="workspace")
    skipped = strided_io.GuardedBytes(4, align=4, device="cuda", name="skipped")
    gh, gh_s = guarded_map((N, C, H, W), out_layouts[0], align, "heatmap gradient")
    gb, gb_s = guarded_map((N, 4, H, W), out_layouts[1], align, "box gradient")
    sc = None if scales is None else torch.tensor(scales, dtype=torch.float64, device="cuda")
    p = loss.loss_params(stride=STRIDE, **settings)
    rc = lib.cnl_detection_loss_grad_f32(hv.ptr, *hv.strides, bv.ptr, *bv.strides, N, C, H, W, gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), G,
                                         ctypes.byref(p), None if sc is None else sc.data_ptr(), gh.ptr if wanted[0] else None, *gh_s,
                                         gb.ptr if wanted[1] else None, *gb_s, skipped.ptr, ws.ptr, nbytes,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "cnl_detection_loss_grad_f32")
    torch.cuda.synchronize()
    assert hv.unchanged() and bv.unchanged()
    for g in (ws, skipped, gh, gb):
        ok, msg = g.verdict()
        assert ok, msg
    outs = []
    for g, s, shape, w in ((gh, gh_s, (N, C, H, W), wanted[0]), (gb, gb_s, (N, 4, H, W), wanted[1])):
        if not w:
            assert g.untouched(), f"{g.name}: not wanted, yet written"
            outs.append(None)
            continue
        a = g.typed(torch.float32).as_strided(shape, s).cpu().numpy()
        assert not np.isnan(a).any(), f"{g.name}: an element was never written"      # (the buffer was all NaN bytes)
        outs.append(a)
    return outs[0], outs[1], int(skipped.result(torch.int32)[0])


@pytest.mark.parametrize("out_layout", OUT_LAYOUTS)
@pytest.mark.parametrize("in_layout", ["nhwc", "nchw", "every_other_channel"])
@pytest.mark.parametrize("name", ["edges", "tiles"])
def test_layouts_on_strided_views_and_guarded_outputs(name, in_layout, out_layout):
    want = expected(name)
    other = OUT_LAYOUTS[(OUT_LAYOUTS.index(out_layout) + 1) % 3]      # the box gradient in another layout than the heatmap gradient
    gh, gb, skipped = launch(name, in_layout, (out_layout, other))
    check(gh, gb, skipped, want, case(name)[3], f"{name} {in_layout} -> {out_layout}")


@pytest.mark.parametrize("name", ["edges", "c81", "iou", "log", "small"])
def test_sixteen_byte_aligned_packed_maps(name):
    """16-byte aligned packed channels-last maps: four elements per lane where W * C is a multiple of 4 (not `small`), one otherwise; the same values."""
    want = expected(name)
    gh, gb, skipped = launch(name, "nhwc", ("nhwc", "nhwc"), align=16)
    check(gh, gb, skipped, want, case(name)[3], name)
    gh4, _, _ = launch(name, "nhwc", ("nhwc", "nchw"), align=4)       # a base that is only 4-byte aligned: one element per lane
    assert gh4.tobytes() == gh.tobytes()


def test_only_one_output_wanted_and_the_scales_come_from_the_device():
    want = expected("edges", 2.0, 0.25)
    gh, none, _ = launch("edges", wanted=(True, False), scales=(2.0, 0.25))
    assert none is None
    none, gb, _ = launch("edges", "nchw", ("nchw", "nchw"), wanted=(False, True), scales=(2.0, 0.25))
    assert none is None
    check(gh, gb, 0, want, case("edges")[3], "edges, scales (2, 0.25)")
    _, _, skipped = launch("edges", wanted=(False, False))
    assert skipped == 0


def test_three_runs_give_the_same_bytes():
    for name in ("tiles", "two_pass"):
        runs = [launch(name, align=16) for _ in range(3)]
        for gh, gb, skipped in runs[1:]:
            assert gh.tobytes() == runs[0][0].tobytes() and gb.tobytes() == runs[0][1].tobytes() and skipped == runs[0][2]
        _, _, out = api(name)                                 # the Python layer's packed tensors and the raw call agree as well
        assert out["heatmap_grad"].cpu().numpy().tobytes() == runs[0][0].tobytes() and out["box_2d_grad"].cpu().numpy().tobytes() == runs[0][1].tobytes()


# ----------------------------------------------------------------------------- agreement with the shipped forward
EPS = 2.0 ** -10


@pytest.mark.parametrize("kind", ["giou", "smooth_l1"])
def test_central_differences_of_the_shipped_forward(kind):
    """Logits and box values at multiples of 2^-6, d in {-1, 0, 1}, eps = 2^-10: (total(x + eps d) - total(x - eps d)) / (2 eps) from
    cnl_detection_loss_f64 equals <grad, d> to rtol 1e-4 (the truncation term is of order eps^2)."""
    settings = dict(box_loss=kind, heatmap_loss_weight=0.5, box_loss_weight=3.0)
    N, C, H, W = 2, 3, 16, 20
    rng = np.random.default_rng(21 + len(kind))
    heat = (np.round(rng.normal(-2.0, 2.0, (N, C, H, W)) * 64) / 64).astype(np.float32)
    box = (np.round(rng.uniform(0.25, 5.0, (N, 4, H, W)) * 64) / 64).astype(np.float32)
    targets = []
    for n in range(N):
        wh = np.round(rng.uniform(6.0, 30.0, (5, 2)) * 8) / 8 + 1 / 16
        c = np.stack([rng.uniform(4, W * 4 - 5, 5), rng.uniform(4, H * 4 - 5, 5)], 1)
        targets.append((np.concatenate([np.round((c - wh / 2) * 8) / 8 + 1 / 32, wh], 1), rng.integers(0, C, 5)))
    assert loss_grad_ref.tie_distance(box, targets, C, **settings) > 2 * EPS * STRIDE        # farther than eps * stride from every tie
    touched = loss_grad_ref.detection_loss_grad(heat, box, targets, **settings)["touched"]
    dh = rng.integers(-1, 2, heat.shape).astype(np.float32)
    db = rng.integers(-1, 2, box.shape).astype(np.float32) * touched[:, None]
    gts = device_targets(pad(targets))
    dev = lambda a: torch.from_numpy(a).cuda().contiguous(memory_format=torch.channels_last)
    hi = cl.detection_loss(dev(heat + EPS * dh), dev(box + EPS * db), gts, stride=STRIDE, **settings)["total"]
    lo = cl.detection_loss(dev(heat - EPS * dh), dev(box - EPS * db), gts, stride=STRIDE, **settings)["total"]
    g = cl.detection_loss_grad(dev(heat), dev(box), gts, stride=STRIDE, heatmap_scale=0.5, box_scale=3.0, **settings)
    fd = float(hi - lo) / (2 * EPS)
    dot = float((g["heatmap_grad"].cpu().numpy().astype(np.float64) * dh).sum() + (g["box_2d_grad"].cpu().numpy().astype(np.float64) * db).sum())
    print(kind, "central difference", fd, "<grad, d>", dot)
    np.testing.assert_allclose(fd, dot, rtol=1e-4, atol=0)


# ----------------------------------------------------------------------------- empty and skipped
def test_a_batch_without_boxes_gives_the_negatives_gradient_over_1():
    rng = np.random.default_rng(3)
    heat = rng.normal(-2.0, 2.0, (2, 3, 16, 20)).astype(np.float32)
    box = rng.uniform(-0.5, 6.0, (2, 4, 16, 20)).astype(np.float32)
    targets = [(np.zeros((0, 4)), np.zeros((0,), np.int64))] * 2
    h, b = torch.from_numpy(heat).cuda(), torch.from_numpy(box).cuda()
    out = cl.detection_loss_grad(h, b, [{"boxes": t[0], "labels": t[1]} for t in targets])
    want = loss_grad_ref.heatmap_dterms(heat, np.zeros_like(heat))           # over max(1, 0) = 1
    within(out["heatmap_grad"].cpu().numpy(), want, "no boxes")
    assert (want > 0).all() and not out["box_2d_grad"].cpu().numpy().any() and int(out["skipped"]) == 0
    # and a batch without images: empty gradients, through autograd too
    h0, b0 = torch.zeros(0, 3, 16, 20, device="cuda", requires_grad=True), torch.zeros(0, 4, 16, 20, device="cuda", requires_grad=True)
    out = cl.detection_loss_grad(h0.detach(), b0.detach(), [])
    assert tuple(out["heatmap_grad"].shape) == (0, 3, 16, 20) and tuple(out["box_2d_grad"].shape) == (0, 4, 16, 20) and int(out["skipped"]) == 0
    res = cl.DetectionLoss()({"heatmap": h0, "box_2d": b0}, [])
    res["total"].backward()
    assert float(res["total"]) == 0.0 and tuple(h0.grad.shape) == (0, 3, 16, 20) and tuple(b0.grad.shape) == (0, 4, 16, 20)


def test_a_skipped_box_is_counted_and_changes_nothing_else():
    heat, box, targets, settings = case("edges")
    boxes, labels, count = (a.copy() for a in pad(targets))
    boxes, labels = np.concatenate([boxes, np.full((2, 1, 4), np.nan)], 1), np.concatenate([labels, np.full((2, 1), -7)], 1)
    boxes[1, 1], labels[1, 1], count[1] = [np.nan, 8.0, 8.0, 8.0], 0, 2
    h = torch.from_numpy(heat).cuda().contiguous(memory_format=torch.channels_last)
    b = torch.from_numpy(box).cuda().contiguous(memory_format=torch.channels_last)
    out = cl.detection_loss_grad(h, b, device_targets((boxes, labels, count)), stride=STRIDE, **settings)
    _, _, clean = api("edges")
    assert int(out["skipped"]) == 1 and int(clean["skipped"]) == 0
    assert torch.equal(out["heatmap_grad"], clean["heatmap_grad"]) and torch.equal(out["box_2d_grad"], clean["box_2d_grad"])


# ----------------------------------------------------------------------------- autograd
def tensors(name, channels_last=True, grad=(True, True)):
    heat, box, targets, settings = case(name)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    h = torch.from_numpy(heat).cuda().contiguous(memory_format=fmt).requires_grad_(grad[0])
    b = torch.from_numpy(box).cuda().contiguous(memory_format=fmt).requires_grad_(grad[1])
    return h, b, [{"boxes": bb, "labels": lab} for bb, lab in targets], settings


def test_the_criterion_returns_detection_loss_and_its_backward_is_detection_loss_grad():
    h, b, listed, settings = tensors("edges")
    criterion = cl.DetectionLoss(stride=STRIDE, **settings)
    res = criterion({"heatmap": h, "box_2d": b}, listed)
    plain = cl.detection_loss(h.detach(), b.detach(), listed, stride=STRIDE, **settings)
    assert set(res) == set(plain)
    for key in plain:
        assert torch.equal(res[key], plain[key]) and res[key].dtype == plain[key].dtype and res[key].shape == plain[key].shape, key
    assert all(res[k].grad_fn is not None for k in ("heatmap", "box_2d", "total")) and not res["per_image"].requires_grad and not res["skipped"].requires_grad
    res["total"].backward()
    direct = cl.detection_loss_grad(h.detach(), b.detach(), listed, stride=STRIDE, heatmap_scale=1.0, box_scale=5.0, **settings)
    assert settings["box_loss_weight"] == 5.0
    assert torch.equal(h.grad, direct["heatmap_grad"]) and torch.equal(b.grad, direct["box_2d_grad"])
    assert h.grad.is_contiguous(memory_format=torch.channels_last) and b.grad.stride() == b.stride()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        res["total"].backward()
    # another combination of the outputs, contiguous inputs
    h, b, listed, settings = tensors("edges", channels_last=False)
    res = criterion({"heatmap": h, "box_2d": b}, listed)
    (2 * res["heatmap"] + 3 * res["box_2d"]).backward()
    direct = cl.detection_loss_grad(h.detach(), b.detach(), listed, stride=STRIDE, heatmap_scale=2.0, box_scale=3.0, **settings)
    assert torch.equal(h.grad, direct["heatmap_grad"]) and torch.equal(b.grad, direct["box_2d_grad"]) and h.grad.is_contiguous()
    # a scale that lives on the device
    dev = cl.detection_loss_grad(h.detach(), b.detach(), listed, stride=STRIDE, heatmap_scale=torch.tensor(2.0, dtype=torch.float64, device="cuda"),
                                 box_scale=3.0, want=("box_2d", "heatmap"), **settings)
    assert torch.equal(dev["heatmap_grad"], direct["heatmap_grad"]) and torch.equal(dev["box_2d_grad"], direct["box_2d_grad"])


def test_one_input_requires_grad_and_no_grad_gives_no_graph():
    for grad in ((True, False), (False, True)):
        h, b, listed, settings = tensors("tiles", grad=grad)
        res = cl.DetectionLoss(stride=STRIDE, **settings)({"heatmap": h, "box_2d": b}, listed)
        res["total"].backward()
        direct = cl.detection_loss_grad(h.detach(), b.detach(), listed, stride=STRIDE, **settings, want=("heatmap",) if grad[0] else ("box_2d",))
        if grad[0]:
            assert b.grad is None and direct["box_2d_grad"] is None and torch.equal(h.grad, direct["heatmap_grad"])
        else:
            assert h.grad is None and direct["heatmap_grad"] is None and torch.equal(b.grad, direct["box_2d_grad"])
    h, b, listed, settings = tensors("tiles")
    criterion = cl.DetectionLoss(stride=STRIDE, **settings)
    with torch.no_grad():
        res = criterion({"heatmap": h, "box_2d": b}, listed)
    assert all(res[k].grad_fn is None and not res[k].requires_grad for k in ("heatmap", "box_2d", "total"))
    plain = criterion({"heatmap": h.detach(), "box_2d": b.detach()}, listed)
    assert plain["total"].grad_fn is None and torch.equal(plain["total"], res["total"])


def test_behind_a_1x1_conv_head_the_weights_receive_the_gradient():
    heat, box, targets, settings = case("edges")
    torch.manual_seed(0)
    head_h, head_b = torch.nn.Conv2d(8, 3, 1).cuda(), torch.nn.Conv2d(8, 4, 1).cuda()
    feat = torch.randn(2, 8, 16, 20, device="cuda").contiguous(memory_format=torch.channels_last)
    listed = [{"boxes": bb, "labels": lab} for bb, lab in targets]
    criterion = cl.DetectionLoss(stride=STRIDE, **settings)
    outputs = {"heatmap": head_h(feat), "box_2d": head_b(feat)}
    res = criterion(outputs, listed)
    res["total"].backward()
    g = cl.detection_loss_grad(outputs["heatmap"].detach(), outputs["box_2d"].detach(), listed, stride=STRIDE, heatmap_scale=1.0, box_scale=5.0, **settings)
    for head, key in ((head_h, "heatmap_grad"), (head_b, "box_2d_grad")):
        want_w = torch.einsum("nohw,nihw->oi", g[key].double(), feat.double())
        assert head.weight.grad is not None and float(head.weight.grad.abs().max()) > 0
        want_b = g[key].double().sum((0, 2, 3))
        # (torch's fp32 sums of N H W = 640 products against float64: 640 * 2^-24 = 4e-5 of the largest entry at worst)
        torch.testing.assert_close(head.weight.grad.double().flatten(1), want_w, rtol=1e-4, atol=1e-4 * float(want_w.abs().max()))
        torch.testing.assert_close(head.bias.grad.double(), want_b, rtol=1e-4, atol=1e-4 * float(want_b.abs().max()))
