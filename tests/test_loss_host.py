"""CPU: the validation loss's rule (tests/loss_ref.py) against the reference's recorded compute_loss / update_heatmap (tests/golden/loss_*.npz, written by
tools/make_golden_loss.py), the argument checks of loss.py, the config-key mapping of both YAML generations, and the C ABI's new symbols."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl
import loss_ref
from centernet_lightning_amd import _lib, loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "loss_*.npz")))
NAMES = [os.path.basename(p)[5:-4] for p in GOLDEN]


def load(path):
    z = np.load(path)
    targets = [(z["boxes"][n, :c], z["labels"][n, :c]) for n, c in enumerate(z["count"])]
    return z, targets, json.loads(str(z["settings"]))


def test_fixtures_cover_the_cases_the_rule_names():
    assert len(GOLDEN) >= 11
    seen = [load(p) for p in GOLDEN]
    settings = [s for _, _, s in seen]
    assert {s.get("box_loss", "giou") for s in settings} == set(loss_ref.BOX_LOSSES)
    assert {s.get("heatmap_loss", "cornernet_focal") for s in settings} == set(loss_ref.HEATMAP_LOSSES)
    assert {s.get("heatmap_target", "cornernet") for s in settings} == set(loss_ref.TARGET_METHODS)
    assert any(s.get("box_multiplier") == 16 for s in settings) and any(s.get("box_log") for s in settings)
    shapes = {tuple(z["heat"].shape) for z, _, _ in seen}
    assert (1, 1, 1, 1) in shapes and (2, 5, 33, 70) in shapes and len(shapes) >= 5
    counts = np.concatenate([z["count"] for z, _, _ in seen])
    assert counts.min() == 0 and counts.max() == 130
    for z, _, _ in seen:                                     # slots beyond the count hold NaN; one tolerance pair for all files
        assert all(np.isnan(z["boxes"][n, c:]).all() for n, c in enumerate(z["count"]))
        assert float(z["tol32"]) == float(seen[0][0]["tol32"]) and float(z["tol64"]) == float(seen[0][0]["tol64"])
        assert 0 < float(z["tol64"]) < float(z["tol32"]) < 1e-6


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_restatement_against_the_reference(path):
    z, targets, settings = load(path)
    N, C, H, W = z["heat"].shape
    out = loss_ref.detection_loss(z["heat"], z["box"], targets, stride=int(z["stride"]), **settings)
    # target map: fp32 bits; at most 1 ulp in at most 1 in 10^4 rendered elements (torch's fp32 exp against a correctly rounded one)
    ref_map = z["target_map"]
    apart = np.abs(out["targets"].view(np.int32).astype(np.int64) - ref_map.view(np.int32).astype(np.int64))
    rendered = max(int(np.count_nonzero(ref_map)), 1)
    assert apart.max(initial=0) <= 1 and int(np.count_nonzero(apart)) * 10 ** 4 <= rendered
    assert np.array_equal(out["targets"] == 0, ref_map == 0)
    # integers: exactly
    assert np.array_equal(out["per_image"][:, 2].astype(np.int64), z["num_dets"]) and np.array_equal(out["per_image"][:, 3].astype(np.int64), z["num_boxes"])
    assert np.array_equal(z["num_dets"], z["count"]) and out["skipped"] == 0
    for n in range(N):
        b = z["boxes"][n, :z["count"][n]] / float(z["stride"])
        centres = np.rint(b[:, :2] + b[:, 2:] / 2).astype(int)
        assert [(r["cx"], r["cy"]) for r in out["records"][n]] == [tuple(c) for c in centres.tolist()]
        assert all(0 <= i < H * W for i in out["samples"][n]) and len(out["samples"][n]) == z["num_boxes"][n]
    # losses: four times the deviation the generator measured over all fixtures
    mine = np.array([out["heatmap"], out["box_2d"], out["total"]])
    print("deviation from the float64 golden", np.abs(mine - z["loss64"]) / np.abs(z["loss64"]), "from the fp32 golden",
          np.abs(mine - z["loss32"].astype(np.float64)) / np.abs(z["loss32"]))
    np.testing.assert_allclose(mine, z["loss64"], rtol=4 * float(z["tol64"]), atol=0)
    np.testing.assert_allclose(mine, z["loss32"].astype(np.float64), rtol=4 * float(z["tol32"]), atol=0)


def test_rule_details():
    # ties to even, both in the centre and in the radius; the radius is never negative
    (r,) = loss_ref.records([[2.0, 6.0, 0.0, 0.0]], [0], 1, 8, 8, stride=4, method="fixed", param=2.5)
    assert (r["cx"], r["cy"], r["rx"], r["ry"]) == (0, 2, 2, 2)
    (r,) = loss_ref.records([[0, 0, 8, 8]], [0], 1, 8, 8, method="fixed", param=-3.0)
    assert (r["rx"], r["ry"]) == (0, 0) and r["den_x"] == np.float32(2 * (1 / 6) ** 2)
    # skipped: non-finite, negative size, centre outside, label outside
    bad = [[np.nan, 0, 4, 4], [0, 0, -1, 4], [100, 0, 4, 4], [0, 0, 4, np.inf], [-9, 0, 4, 4]]
    assert [r["state"] for r in loss_ref.records(bad, [0] * 5, 1, 8, 8)] == [0] * 5
    assert [r["state"] for r in loss_ref.records([[0, 0, 4, 4]] * 2, [-1, 1], 1, 8, 8)] == [0, 0]
    # a centre ON the right edge: counted, its samples are column W - 1, and the part of its window inside the map is rendered without a peak
    recs = loss_ref.records([[28, 8, 8, 8]], [0], 1, 8, 8, method="fixed", param=2.0)
    assert recs[0]["cx"] == 8 and loss_ref.samples(recs[0], 8, 8) == [(7, 2), (7, 3), (7, 4)]
    m = loss_ref.render(recs, 1, 8, 8)
    assert m.max() < 1 and np.count_nonzero(m) == 10 and np.count_nonzero(m[:, :, :6]) == 0
    # a peak is exactly one; the cut at eps removes the far tail
    recs = loss_ref.records([[8, 8, 8, 8]], [0], 1, 16, 16, method="fixed", param=9.0)
    m = loss_ref.render(recs, 1, 16, 16)
    assert m[0, 3, 3] == 1.0 and m.dtype == np.float32 and (m[m > 0] >= np.finfo(np.float32).eps).all()


# ----------------------------------------------------------------------------- the Python layer
def _maps(N=2, C=3, H=4, W=5):
    return torch.zeros(N, C, H, W), torch.zeros(N, 4, H, W)


def _targets(N=2):
    return [{"boxes": [[0.0, 0.0, 4.0, 4.0]], "labels": [0]} for _ in range(N)]


@pytest.mark.parametrize("kwargs, match", [
    (dict(heatmap_target="gaussian"), "heatmap_target must be one of"),
    (dict(heatmap_target_params={"alpha": 0.5}), "may hold 'min_overlap' only"),
    (dict(heatmap_target_params={"min_overlap": 1.5}), r"min_overlap must lie in \(0, 1\)"),
    (dict(heatmap_loss="focal"), "heatmap_loss must be one of"),
    (dict(box_loss="L2Loss"), "box_loss must be one of"),
    (dict(stride=0), "stride must be a finite positive number"),
    (dict(box_loss_weight=float("nan")), "box_loss_weight must be a finite number"),
    (dict(box_multiplier="16"), "box_multiplier must be a finite number"),
])
def test_settings_are_checked_before_anything_else(kwargs, match):
    heat, box = _maps()
    with pytest.raises(ValueError, match=match):
        cl.detection_loss(heat, box, _targets(), **kwargs)
    with pytest.raises(ValueError, match=match):
        cl.LossMeter(**kwargs)


def test_maps_and_targets_are_checked_before_any_launch():
    heat, box = _maps()
    with pytest.raises(ValueError, match="heatmap must be a float32 tensor"):
        cl.detection_loss(heat.double(), box, _targets())
    with pytest.raises(ValueError, match=r"needs box_2d \[2, 4, 4, 5\]"):
        cl.detection_loss(heat, box[:, :2], _targets())
    with pytest.raises(RuntimeError, match="HIP devices only"):         # well-formed CPU tensors: no CPU fallback
        cl.detection_loss(heat, box, _targets())
    with pytest.raises(ValueError, match="2 images of outputs against 1 of targets"):
        loss._targets(_targets(1), 2, 3, 4, 5, 4.0, "detection_loss")
    with pytest.raises(ValueError, match="must be a dict with 'boxes', 'labels'"):
        loss._targets([{"boxes": []}, {}], 2, 3, 4, 5, 4.0, "detection_loss")
    with pytest.raises(ValueError, match=r"expected \[n, 4\] and \[n\]"):
        loss._targets([{"boxes": [[0, 0, 1, 1]], "labels": [0, 1]}] * 2, 2, 3, 4, 5, 4.0, "detection_loss")
    with pytest.raises(ValueError, match="at most 1024 per image"):
        loss._targets([{"boxes": np.zeros((1025, 4)), "labels": np.zeros(1025)}], 1, 3, 4, 5, 4.0, "detection_loss")
    for box_, label in (([0, 0, np.nan, 4], 0), ([0, 0, -4, 4], 0), ([40, 0, 4, 4], 0), ([0, 0, 4, 4], 3), ([0, 0, 4, 4], -1)):
        with pytest.raises(ValueError, match="cannot be a target"):
            loss._targets([{"boxes": [box_], "labels": [label]}], 1, 3, 4, 5, 4.0, "detection_loss")
    with pytest.raises(ValueError, match="device targets need 'boxes'"):
        loss._targets({"boxes": torch.zeros(2, 1, 4)}, 2, 3, 4, 5, 4.0, "detection_loss")
    with pytest.raises(ValueError, match="targets 'boxes' must be torch.float64"):
        loss._targets((torch.zeros(2, 1, 4), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)), 2, 3, 4, 5, 4.0, "detection_loss")
    with pytest.raises(ValueError, match=r"expected target boxes \[2,Gmax,4\]"):
        loss._targets((torch.zeros(3, 1, 4, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)), 2, 3, 4, 5, 4.0,
                      "detection_loss")
    # the list form is padded: centres ON the edge are targets
    dev, (b, lab, cnt), G = loss._targets([{"boxes": [[16, 12, 8, 8], [0, 0, 4, 4]], "labels": [2, 0]}, {"boxes": [], "labels": []}], 2, 3, 4, 5, 4.0, "x")
    assert dev is None and G == 2 and b.shape == (2, 2, 4) and b.dtype == np.float64 and cnt.tolist() == [2, 0] and lab.dtype == np.int64
    with pytest.raises(ValueError, match="num_classes must be an int"):
        cl.render_targets(_targets(), 2.5, 4, 5)
    with pytest.raises(ValueError, match="outside"):
        cl.render_targets(_targets(), 3, 0, 5)
    with pytest.raises(ValueError, match="outputs must be the dict of get_encoded_outputs"):
        cl.LossMeter().update((heat, box), _targets())
    with pytest.raises(RuntimeError, match="nothing has been measured"):
        cl.LossMeter().get_metrics()
    with pytest.raises(ValueError, match="merge expects"):
        cl.LossMeter().merge({"sums": None})


def test_config_keys_of_both_generations():
    gen_a = {"heatmap": {"num_classes": 3, "target_method": "ttfnet", "loss_function": "quality", "loss_weight": 2},
             "box_2d": {"loss_function": "smooth_l1", "loss_weight": 0.5}, "reid": {"loss_function": "ce", "loss_weight": 1}}
    assert loss.settings_from_config(gen_a) == {"heatmap_target": "ttfnet", "heatmap_loss": "quality", "heatmap_loss_weight": 2, "box_loss": "smooth_l1",
                                                "box_loss_weight": 0.5}
    gen_b = dict(heatmap_loss="CornerNetFocalLoss", box_loss="GIoULoss", heatmap_loss_weight=1.0, box_loss_weight=5, heatmap_target="cornernet",
                 heatmap_target_params={"min_overlap": 0.4}, num_detections=100)
    got = loss.settings_from_config({"heatmap": {"num_classes": 3}, "box_2d": {}}, **gen_b)
    assert got == {k: v for k, v in gen_b.items() if k != "num_detections"}
    assert loss.settings_from_config({"heatmap": {"num_classes": 3}, "box_2d": None}) == {}
    with pytest.raises(ValueError, match="box_loss must be one of"):
        loss.settings_from_config({"heatmap": {}, "box_2d": {"loss_function": "huber"}})
    for a, b in (("cornernet_focal", "CornerNetFocalLoss"), ("quality", "QualityFocalLoss")):
        assert loss.HEATMAP_LOSSES[a] == loss.HEATMAP_LOSSES[b]
    for a, b in zip(loss_ref.BOX_LOSSES, ("L1Loss", "SmoothL1Loss", "IoULoss", "GIoULoss", "DIoULoss", "CIoULoss")):
        assert loss.BOX_LOSSES[a] == loss.BOX_LOSSES[b] == loss_ref.BOX_LOSSES.index(a)
    # the model reads them where it is built, and hands stride / box_log / box_multiplier over itself
    cfg = {"model": {"backbone": {"name": "resnet18"}, "neck": {"name": "fpn"}, "box_multiplier": 16.0, "box_loss": "L1Loss", "box_loss_weight": 0.1,
                     "output_heads": {"heatmap": {"num_classes": 2, "target_method": "ttfnet"}, "box_2d": {"loss_function": "giou", "loss_weight": 5}}}}
    try:
        model = cl.build_centernet(cfg)
    except Exception as e:                                   # (a backbone / neck spelling this tree does not build is not this test's subject)
        pytest.fail(f"build_centernet on the loss config: {e}")
    assert model.loss_settings == {"heatmap_target": "ttfnet", "box_loss": "L1Loss", "box_loss_weight": 0.1}
    kw = model._loss_kwargs(None)
    assert kw["stride"] == model.stride and kw["box_multiplier"] == 16.0 and kw["box_log"] is False
    assert model.loss_meter().settings == kw


def test_symbols_and_params_struct():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    for name in ("cnl_detection_loss_workspace_bytes", "cnl_detection_loss_f64"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "typedef struct cnl_loss_params" in header
    assert lib.cnl_sizeof_params(4) == ctypes.sizeof(_lib.LossParams) == 72
    # the record, partial and per-image sections: 32 bytes per slot, 8 per 8 x 32 tile, 32 per image
    assert lib.cnl_detection_loss_workspace_bytes(2, 3, 33, 70) == 2 * 3 * 32 + 2 * 5 * 3 * 8 + 2 * 32
    assert lib.cnl_detection_loss_workspace_bytes(1, 1025, 4, 4) == 0 and lib.cnl_detection_loss_workspace_bytes(1, 1, 0, 4) == 0
    p = loss.loss_params(heatmap_target="ttfnet", box_loss="CIoULoss", box_multiplier=16)
    assert (p.target_method, p.target_param, p.box_loss, p.box_multiplier, p.hm_alpha, p.hm_beta) == (1, 0.54, 5, 16.0, 2.0, 4.0)
    # argument errors come back as codes, without a device
    args = [None, 0, 0, 0, 0, None, 0, 0, 0, 0, 1, 1, 4, 4, None, None, None, 1, ctypes.byref(p), None, 0, 0, 0, 0, None, None, None, None, 0, None]
    assert lib.cnl_detection_loss_f64(*args) == _lib.CNL_E_BAD_ARG and "nothing to do" in _lib.last_error()
    args[18] = None
    assert lib.cnl_detection_loss_f64(*args) == _lib.CNL_E_BAD_ARG and "null params" in _lib.last_error()
    p.box_loss = 9
    args[18] = ctypes.byref(p)
    assert lib.cnl_detection_loss_f64(*args) == _lib.CNL_E_BAD_ARG and "box_loss = 9" in _lib.last_error()
