"""GPU: the validation loss (cnl_detection_loss_f64, csrc/det_loss.hip; loss.py) against tests/loss_ref.py.

Tolerances.  Counts and the target map's zero set and peaks are exact.  The target map may differ by 1 ulp in at most 1 in 10^4 rendered elements
(the device's float64 exp against numpy's, rounded to fp32).  Rows and totals: rtol 1e-8 — the terms are non-negative, float64 accumulation over
at most 1e5 elements costs at most 1e-11, and an fp32-ulp difference in a capped handful of targets moves a sum by less than 1e-9.  With box_log
the device's and the host's fp32 exp may differ by an ulp or two of the box size, and the inputs keep every |pred - target| above 1/100 of that
size: rtol 1e-5 on the box sums.

Shapes are the smallest that reach each path: H x W in 1x1, 3x5, 16x20, 33x70 (tiles are 8 x 32: none is a multiple, the last tile is partial in
both directions, 33x70 has 5 x 3 tiles), C in 1, 2, 3, 80, 81, boxes per image 0, 1, 9 and PASS_SLOTS + 44 (two staging passes)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import loss_ref
import strided_io
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, loss

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")
PASS_SLOTS = 256              # csrc/det_loss.hip: target slots staged per pass
TILE_H, TILE_W = 8, 32
STRIDE = 4
RTOL, RTOL_LOG = 1e-8, 1e-5


def boxes_at(centres, sizes):
    """x y w h in input pixels with the given centres and sizes in map pixels."""
    c, s = np.asarray(centres, np.float64) * STRIDE, np.asarray(sizes, np.float64) * STRIDE
    return np.concatenate([c - s / 2, s], 1)


def random_targets(rng, m, C, H, W, max_size=10.0, min_size=0.5):
    centres = np.stack([rng.integers(0, W, m), rng.integers(0, H, m)], 1) + rng.uniform(-0.4, 0.4, (m, 2))
    return boxes_at(centres, rng.uniform(min_size, max_size, (m, 2))), rng.integers(0, C, m).astype(np.int64)


CASES = {
    # name: (seed, (N, C, H, W), boxes per image, settings)
    "pixel": (1, (1, 1, 1, 1), [1], dict(heatmap_target="fixed", heatmap_target_params={"r": 0.0}, box_loss="l1")),                 # radius 0
    "small": (2, (2, 2, 3, 5), [1, 0], dict(heatmap_target="ttfnet", heatmap_target_params={"alpha": 3.0}, heatmap_loss="quality", box_loss="l1")),
    "edges": (3, (2, 3, 16, 20), [9, 1], dict(box_loss="giou", box_loss_weight=5.0)),
    "c80": (4, (1, 80, 33, 70), [9], dict(box_loss="iou")),
    "c81": (5, (2, 81, 16, 20), [9, 0], dict(heatmap_loss="quality", box_loss="smooth_l1", box_multiplier=16.0, heatmap_loss_weight=0.5)),
    "two_pass": (6, (1, 2, 16, 20), [PASS_SLOTS + 44], dict(box_loss="diou", heatmap_target="fixed")),
    "tiles": (7, (2, 3, 33, 70), [9, 9], dict(box_loss="ciou", heatmap_target="ttfnet")),
    "log": (8, (1, 3, 16, 20), [9], dict(box_log=True, box_loss="l1")),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (heat [N,C,H,W] f32, box [N,4,H,W] f32, [(boxes, labels)], padded (boxes [N,G,4] with NaN beyond the count, labels, count), settings)"""
    seed, (N, C, H, W), counts, settings = CASES[name]
    rng = np.random.default_rng(seed)
    targets = []
    for n in range(N):
        # (box_log: predictions reach at most 4 e^1.2 = 13.3 input pixels from a sample, targets of 14 to 18 map pixels at least 28 from their centre)
        b, lab = random_targets(rng, counts[n], C, H, W, *((18.0, 14.0) if name == "log" else ()))
        if name == "small" and n == 0:
            b, lab = boxes_at([[2.0, 1.0]], [[4.0, 3.0]]), np.array([1])            # ttfnet alpha 3: radii (6, 4) on a 3 x 5 map
        if name == "edges" and n == 0:
            # centres at 0, W - 1, ON W and ON H; two same-class Gaussians that overlap, and one of another class over them
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
    G = max([1] + counts)
    boxes, labels = np.full((N, G, 4), np.nan), np.full((N, G), -7, np.int64)
    for n, (b, lab) in enumerate(targets):
        boxes[n, :len(lab)], labels[n, :len(lab)] = b, lab
    return heat, box, targets, (boxes, labels, np.array(counts, np.int32)), settings


@functools.lru_cache(maxsize=None)
def expected(name):
    heat, box, targets, _, settings = case(name)
    return loss_ref.detection_loss(heat, box, targets, stride=STRIDE, **settings)


def device_targets(padded):
    return tuple(torch.from_numpy(a).cuda() for a in padded)


def check_map(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    apart = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    rendered = max(int(np.count_nonzero(want)), 1)
    assert apart.max(initial=0) <= 1 and int(np.count_nonzero(apart)) * 10 ** 4 <= rendered, (int(apart.max(initial=0)), int(np.count_nonzero(apart)), rendered)
    assert np.array_equal(got == 0, want == 0)
    assert np.array_equal(got == 1, want == 1)


def check_result(rows, totals, skipped, want, box_rtol=RTOL):
    rows, totals = np.asarray(rows, np.float64), np.asarray(totals, np.float64)
    print("rows", rows.tolist(), "totals", totals.tolist(), "expected", want["per_image"].tolist(), [want["heatmap"], want["box_2d"], want["total"]])
    assert np.array_equal(rows[:, 2:], want["per_image"][:, 2:])                     # counts: exactly
    assert int(skipped) == want["skipped"]
    np.testing.assert_allclose(rows[:, 0], want["per_image"][:, 0], rtol=RTOL, atol=0)
    np.testing.assert_allclose(rows[:, 1], want["per_image"][:, 1], rtol=box_rtol, atol=0)
    np.testing.assert_allclose(totals[0], want["heatmap"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(totals[1:], [want["box_2d"], want["total"]], rtol=box_rtol, atol=0)


def api(name, **kw):
    heat, box, _, padded, settings = case(name)
    h = torch.from_numpy(heat).cuda().contiguous(memory_format=torch.channels_last)
    b = torch.from_numpy(box).cuda().contiguous(memory_format=torch.channels_last)
    return cl.detection_loss(h, b, device_targets(padded), stride=STRIDE, **settings, **kw)


# ----------------------------------------------------------------------------- the Python layer, the engine's layout
@pytest.mark.parametrize("name", list(CASES))
def test_detection_loss_against_the_restatement(name):
    want = expected(name)
    out = api(name, return_targets=True)
    assert out["heatmap"].dim() == 0 and out["heatmap"].dtype == torch.float64 and out["per_image"].shape == (len(want["per_image"]), 4)
    assert out["targets"].is_contiguous(memory_format=torch.channels_last) or out["targets"].is_contiguous()
    check_map(out["targets"].cpu().numpy(), want["targets"])
    check_result(out["per_image"].cpu().numpy(), [float(out["heatmap"]), float(out["box_2d"]), float(out["total"])], out["skipped"],
                 want, RTOL_LOG if CASES[name][3].get("box_log") else RTOL)


def test_log_inputs_keep_the_differences_large():
    """The premise of RTOL_LOG: every |pred - target| of the box_log case is above 1/100 of the box size."""
    _, box, targets, _, settings = case("log")
    want = expected("log")
    for rec, b in zip(want["records"][0], targets[0][0]):
        for (x, y) in loss_ref.samples(rec, 16, 20):
            pred, tgt = loss_ref.decode_box(box[0], x, y, STRIDE, True, 1.0), loss_ref.box_target(b)
            assert (np.abs(pred.astype(np.float64) - tgt) > np.abs(pred).max() / 100).all()


def test_two_passes_are_needed():
    _, _, targets, _, _ = case("two_pass")
    recs = expected("two_pass")["records"][0]
    touching = sum(1 for r in recs if r["state"] and r["cx"] - r["rx"] < TILE_W and r["cy"] - r["ry"] < TILE_H)
    assert len(recs) > PASS_SLOTS and touching > PASS_SLOTS      # slots beyond the first pass reach the first tile too
    assert any(r["cx"] - r["rx"] < TILE_W and r["cy"] - r["ry"] < TILE_H for r in recs[PASS_SLOTS:])


def test_render_targets_and_the_list_form():
    heat, box, targets, padded, settings = case("edges")
    want = expected("edges")
    kw = {k: settings[k] for k in ("heatmap_target", "heatmap_target_params") if k in settings}
    listed = [{"boxes": b, "labels": lab} for b, lab in targets]
    for tg in (listed, device_targets(padded)):
        m = cl.render_targets(tg, 3, 16, 20, stride=STRIDE, **kw)
        assert tuple(m.shape) == (2, 3, 16, 20) and m.dtype == torch.float32
        check_map(m.cpu().numpy(), want["targets"])
    # peaks: exactly one at every centre inside the map
    got = m.cpu().numpy()
    for rec in want["records"][0]:
        if rec["cx"] < 20 and rec["cy"] < 16:
            assert got[0, rec["label"], rec["cy"], rec["cx"]] == 1.0
    a = api("edges")
    h, b = torch.from_numpy(heat).cuda(), torch.from_numpy(box).cuda()
    c = cl.detection_loss(h.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last), listed, stride=STRIDE, **settings)
    assert torch.equal(a["per_image"], c["per_image"]) and float(a["total"]) == float(c["total"])      # the two target forms: the same bits


# ----------------------------------------------------------------------------- the C ABI on strided views, guarded outputs, exact workspace
LAYOUT_PATHS = {"nhwc_wide": "channel stride 1", "nhwc_off1": "channel stride 1", "nchw_window_odd": "W stride 1", "every_other_channel": "generic",
                "every_other_pixel_nchw": "generic"}


def launch(name, layout, map_layout=None, heat=None):
    """One raw call.  -> (rows, totals, skipped, target map or None)"""
    heat0, box, _, padded, settings = case(name)
    heat = heat0 if heat is None else heat
    N, C, H, W = heat.shape
    lib = _lib.load()
    hv = strided_io.StridedView(torch.from_numpy(heat), layout, poison="nan", device="cuda", name="heat")
    bv = strided_io.StridedView(torch.from_numpy(box), layout, poison="nan", device="cuda", name="box")
    tv = strided_io.StridedView(torch.full((N, C, H, W), -3.0), map_layout, poison="nan", device="cuda", name="target map") if map_layout else None
    gts = device_targets(padded)
    G = padded[0].shape[1]
    nbytes = lib.cnl_detection_loss_workspace_bytes(N, G, H, W)
    assert nbytes > 0
    ws = strided_io.GuardedBytes(nbytes, align=16, device="cuda", name="workspace")
    rows = strided_io.GuardedBytes(N * 32, align=8, device="cuda", name="per_image")
    totals = strided_io.GuardedBytes(24, align=8, device="cuda", name="totals")
    skipped = strided_io.GuardedBytes(4, align=4, device="cuda", name="skipped")
    p = loss.loss_params(stride=STRIDE, **settings)
    rc = lib.cnl_detection_loss_f64(hv.ptr, *hv.strides, bv.ptr, *bv.strides, N, C, H, W, gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), G,
                                    ctypes.byref(p), tv.ptr if tv else None, *(tv.strides if tv else (0, 0, 0, 0)), rows.ptr, totals.ptr, skipped.ptr,
                                    ws.ptr, nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "cnl_detection_loss_f64")
    torch.cuda.synchronize()
    assert hv.unchanged() and bv.unchanged()
    for g in (ws, rows, totals, skipped):
        ok, msg = g.verdict()
        assert ok, msg
    tmap = None
    if tv:
        tmap = tv.view.cpu().numpy().copy()
        assert not np.isnan(tmap).any() and (tmap != -3.0).all()                   # every element received its target
        tv.view.copy_(tv.snapshot.as_strided(tv.view.shape, tv.view.stride(), tv.view.storage_offset()))
        assert tv.unchanged(), "target map: written outside the view"
    return rows.result(torch.float64, (N, 4)).numpy(), totals.result(torch.float64).numpy(), int(skipped.result(torch.int32)[0]), tmap


@pytest.mark.parametrize("layout", list(LAYOUT_PATHS))
@pytest.mark.parametrize("name", ["small", "edges", "c81"])
def test_layout_paths_on_strided_views(name, layout):
    want = expected(name)
    rows, totals, skipped, tmap = launch(name, layout, map_layout="nchw_window" if layout.startswith("nhwc") else "nhwc_off2")
    check_map(tmap, want["targets"])
    check_result(rows, totals, skipped, want)


@pytest.mark.parametrize("layout", ["nhwc", "nchw", "every_other_channel"])
def test_a_planted_logit_moves_the_loss_by_what_the_restatement_says(layout):
    """+20 at a tile corner, in the last row, the last column and the last channel: each alone is about 20 of a sum of about 100, so a skipped edge shows."""
    heat, box, targets, _, settings = case("tiles")
    base = expected("tiles")
    N, C, H, W = heat.shape
    for (n, c, y, x) in ((0, 0, TILE_H, TILE_W), (1, 1, H - 1, 5), (0, 1, 3, W - 1), (1, C - 1, 2 * TILE_H + 1, 2 * TILE_W + 1), (1, 0, H - 1, W - 1)):
        planted = heat.copy()
        planted[n, c, y, x] = 20.0
        t = base["targets"][n, c, y, x]
        delta = (loss_ref.heatmap_terms(np.float32(20.0), t, "cornernet_focal") - loss_ref.heatmap_terms(heat[n, c, y, x], t, "cornernet_focal"))
        rows, totals, _, _ = launch("tiles", layout, heat=planted)
        want = base["per_image"][:, 0].copy()
        want[n] += float(delta)
        assert float(delta) > 10.0
        np.testing.assert_allclose(rows[:, 0], want, rtol=RTOL, atol=0)


def test_three_runs_give_the_same_bits_and_an_image_alone_gives_its_row():
    heat, box, _, padded, settings = case("tiles")
    runs = [launch("tiles", "nhwc") for _ in range(3)]
    for rows, totals, skipped, _ in runs[1:]:
        assert rows.tobytes() == runs[0][0].tobytes() and totals.tobytes() == runs[0][1].tobytes() and skipped == runs[0][2]
    whole = api("tiles")
    assert whole["per_image"].cpu().numpy().tobytes() == runs[0][0].tobytes()         # packed channels-last and the raw call agree as well
    dev = device_targets(padded)
    for n in range(heat.shape[0]):
        h = torch.from_numpy(heat[n:n + 1]).cuda().contiguous(memory_format=torch.channels_last)
        b = torch.from_numpy(box[n:n + 1]).cuda().contiguous(memory_format=torch.channels_last)
        alone = cl.detection_loss(h, b, tuple(t[n:n + 1] for t in dev), stride=STRIDE, **settings)
        assert torch.equal(alone["per_image"][0], whole["per_image"][n])


def test_a_skipped_box_is_counted_and_changes_nothing_else():
    heat, box, targets, padded, settings = case("edges")
    boxes, labels, count = (a.copy() for a in padded)
    G = boxes.shape[1]
    boxes, labels = np.concatenate([boxes, np.full((2, 1, 4), np.nan)], 1), np.concatenate([labels, np.full((2, 1), -7)], 1)
    boxes[1, 1], labels[1, 1], count[1] = [400.0, 8.0, 8.0, 8.0], 0, 2              # its centre lies outside the map
    assert G == 9
    h = torch.from_numpy(heat).cuda().contiguous(memory_format=torch.channels_last)
    b = torch.from_numpy(box).cuda().contiguous(memory_format=torch.channels_last)
    out = cl.detection_loss(h, b, device_targets((boxes, labels, count)), stride=STRIDE, **settings)
    clean = api("edges")
    assert int(out["skipped"]) == 1 and int(clean["skipped"]) == 0
    assert torch.equal(out["per_image"], clean["per_image"]) and float(out["total"]) == float(clean["total"])
    meter = cl.LossMeter(stride=STRIDE, **settings)
    meter.update({"heatmap": h, "box_2d": b}, device_targets((boxes, labels, count)))
    with pytest.raises(ValueError, match="1 target box"):
        meter.get_metrics()
    with pytest.raises(ValueError, match="cannot be a target"):                       # the list form finds it before the upload
        cl.detection_loss(h, b, [{"boxes": targets[0][0], "labels": targets[0][1]}, {"boxes": boxes[1, :2], "labels": labels[1, :2]}], stride=STRIDE, **settings)


def test_loss_meter_shards_merge_to_one_meter():
    batches = []
    for name in ("edges", "tiles"):
        heat, box, _, padded, _ = case(name)
        batches.append(({"heatmap": torch.from_numpy(heat).cuda().contiguous(memory_format=torch.channels_last),
                         "box_2d": torch.from_numpy(box).cuda().contiguous(memory_format=torch.channels_last)}, device_targets(padded)))
    settings = dict(stride=STRIDE, box_loss="giou", box_loss_weight=5.0)
    one, a, b = cl.LossMeter(**settings), cl.LossMeter(**settings), cl.LossMeter(**settings)
    for out, tg in batches:
        one.update(out, tg)
    a.update(*batches[0])
    b.update(*batches[1])
    a.merge(b.state())
    got = one.get_metrics()
    assert a.get_metrics() == got and list(got) == ["heatmap_loss", "box_2d_loss", "total_loss"] and a.num_batches == 2
    refs = [loss_ref.detection_loss(case(n)[0], case(n)[1], case(n)[2], stride=STRIDE, box_loss="giou", box_loss_weight=5.0) for n in ("edges", "tiles")]
    for key, name in (("heatmap", "heatmap_loss"), ("box_2d", "box_2d_loss"), ("total", "total_loss")):
        np.testing.assert_allclose(got[name], (refs[0][key] * 2 + refs[1][key] * 2) / 4, rtol=RTOL, atol=0)
    one.reset()
    one.update(*batches[0])
    np.testing.assert_allclose(one.get_metrics()["total_loss"], refs[0]["total"], rtol=RTOL, atol=0)


def test_model_compute_loss_is_detection_loss_on_its_outputs():
    import recipes
    import ref_cpu
    cfg = cl.load_config(os.path.join(CONFIGS, "resnet34_fpn.yaml"))
    cfg["model"]["output_heads"]["heatmap"].update(target_method="ttfnet", loss_function="quality", loss_weight=2)
    cfg["model"]["output_heads"]["box_2d"].update(loss_function="diou", loss_weight=0.5)
    cfg["model"]["box_multiplier"] = 16.0
    model = cl.build_centernet(cfg)
    model.load_state_dict(ref_cpu.synth_state_dict(model.state_dict(), seed=0, calib_shape=(1, 3, 64, 64)))
    model = model.cuda()
    outputs = model.get_encoded_outputs(recipes.images(5, (2, 3, 64, 64)).cuda())
    N, C, H, W = outputs["heatmap"].shape
    rng = np.random.default_rng(9)
    targets = [{"boxes": b, "labels": lab} for b, lab in (random_targets(rng, m, C, H, W, 6.0) for m in (5, 2))]
    got = model.compute_loss(outputs, targets)
    kw = dict(stride=model.stride, heatmap_target="ttfnet", heatmap_loss="quality", box_loss="diou", heatmap_loss_weight=2, box_loss_weight=0.5,
              box_multiplier=16.0)
    direct = cl.detection_loss(outputs["heatmap"], outputs["box_2d"], targets, **kw)
    for key in ("heatmap", "box_2d", "total", "per_image", "skipped"):
        assert torch.equal(got[key], direct[key])
    want = loss_ref.detection_loss(outputs["heatmap"].cpu().numpy(), outputs["box_2d"].cpu().numpy(), [(t["boxes"], t["labels"]) for t in targets], **kw)
    check_result(got["per_image"].cpu().numpy(), [float(got["heatmap"]), float(got["box_2d"]), float(got["total"])], got["skipped"], want)
    meter = model.loss_meter()
    meter.update(outputs, targets)
    assert meter.get_metrics()["total_loss"] == float(got["total"])
