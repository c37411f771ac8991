"""CPU: the gradient rule of the detection loss (tests/loss_grad_ref.py) against the reference's recorded autograd gradients
(tests/golden/grad_loss_*.npz, written by tools/make_golden_loss_grad.py) and against central differences of tests/loss_ref.py's value, the argument
checks of loss.detection_loss_grad / DetectionLoss, and the C ABI's two new symbols."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl
import loss_grad_ref
import loss_ref
from centernet_lightning_amd import _lib, loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "grad_loss_*.npz")))
NAMES = [os.path.basename(p)[10:-4] for p in GOLDEN]
GRADS = ("d_heatmap_d_heat", "d_heatmap_d_box", "d_box_d_heat", "d_box_d_box")


def load(path):
    z = np.load(path)
    targets = [(z["boxes"][n, :c], z["labels"][n, :c]) for n, c in enumerate(z["count"])]
    return z, targets, json.loads(str(z["settings"]))


def test_fixtures_cover_the_cases_the_rule_names():
    seen = [load(p) for p in GOLDEN]
    settings = [s for _, _, s in seen]
    assert {s.get("box_loss", "giou") for s in settings} == set(loss_ref.BOX_LOSSES)
    assert {s.get("heatmap_loss", "cornernet_focal") for s in settings} == set(loss_ref.HEATMAP_LOSSES)
    assert {s.get("heatmap_target", "cornernet") for s in settings} == set(loss_ref.TARGET_METHODS)
    assert any(s.get("box_multiplier") == 16 for s in settings) and any(s.get("box_log") for s in settings)
    assert any(s.get("heatmap_target_params") == {"r": 0.0} for s in settings)
    assert {"edges", "ties", "ties_smooth", "ties_iou", "ties_giou", "ties_diou", "ties_ciou", "ties_zero_giou"} <= set(NAMES)
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "loss_*.npz")))
    for (z, _, _), path in zip(seen, GOLDEN):
        assert float(z["tol64"]) == float(seen[0][0]["tol64"]) and 0 < float(z["tol64"]) < 1e-5
        assert os.path.getsize(path) <= largest
        assert all(z[k].dtype == np.float64 for k in GRADS) and z["d_heatmap_d_heat"].shape == z["heat"].shape and z["d_box_d_box"].shape == z["box"].shape


def planted(name):
    """The decoded box minus the target at every sample of the first box of a ties fixture, and the raw box values at all samples."""
    z, targets, st = load(GOLDEN[NAMES.index(name)])
    N, C, H, W = z["heat"].shape
    recs = loss_ref.records(*targets[0], C, H, W, int(z["stride"]), st["heatmap_target"], st["heatmap_target_params"]["r"])
    diffs = [loss_ref.decode_box(z["box"][0], x, y, int(z["stride"])).astype(np.float64) - loss_ref.box_target(targets[0][0][0])
             for (x, y) in loss_ref.samples(recs[0], H, W)]
    raw = [z["box"][0, :, y, x] for r in recs for (x, y) in loss_ref.samples(r, H, W)]
    return z, np.array(diffs), np.array(raw)


def test_the_ties_fixtures_hold_the_points_they_are_named_for():
    z, d, raw = planted("ties")                              # l1: differences of exactly 0; the clamp at exactly 0 and below; sigmoid(x) == t
    assert (d[:, 0] == 0).all() and (d[:, 3] == 0).all() and (d[:, 1] != 0).all() and len(d) == 9
    assert (raw == 0).any() and (raw < 0).any()
    tmap = loss_ref.render(loss_ref.records(z["boxes"][0], z["labels"][0], 2, 12, 16, 4, "fixed", 2.0), 2, 12, 16)
    with np.errstate(over="ignore"):
        p = 1 / (1 + np.exp(-z["heat"][0].astype(np.float64)))
    assert ((tmap == 1) & (p == 1)).any() and ((tmap == 0) & (p == 0)).any()
    _, d, _ = planted("ties_smooth")
    assert (np.abs(d[:, 0]) == 1).all() and (np.abs(d[:, 1]) == 1).all()
    for kind in ("iou", "giou", "diou", "ciou"):
        _, d, raw = planted(f"ties_{kind}")                  # corners that equal the target's: maximum / minimum ties
        assert (d[:, 0] == 0).all() and (d[:, 2] == 0).all() and (raw == 0).any() and (raw < 0).any()
        z, targets, st = load(GOLDEN[NAMES.index(f"ties_zero_{kind}")])
        t = loss_ref.box_target(targets[0][0][0])
        preds = {(x, y): loss_ref.decode_box(z["box"][0], x, y, 4) for (x, y) in ((6, 4), (4, 5), (6, 5))}
        assert preds[(6, 4)][0] == t[2] and preds[(4, 5)][1] == t[3] and preds[(6, 5)][1] == t[3]      # intersections of width / height exactly 0


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_restatement_against_the_reference(path):
    z, targets, settings = load(path)
    stride, tol = int(z["stride"]), 4 * float(z["tol64"])
    heat_only = loss_grad_ref.detection_loss_grad(z["heat"], z["box"], targets, stride=stride, heatmap_scale=1.0, box_scale=0.0, **settings)
    box_only = loss_grad_ref.detection_loss_grad(z["heat"], z["box"], targets, stride=stride, heatmap_scale=0.0, box_scale=1.0, **settings)
    mine = dict(zip(GRADS, (heat_only["heatmap_grad64"], heat_only["box_2d_grad64"], box_only["heatmap_grad64"], box_only["box_2d_grad64"])))
    for key in GRADS:
        ref = z[key]
        scale = np.abs(ref).max()
        print(key, "max|ref|", scale, "deviation", (np.abs(mine[key] - ref).max() / scale) if scale else 0.0, "allowed", tol)
        if scale == 0:
            assert not mine[key].any()
        else:
            assert np.abs(mine[key] - ref).max() <= tol * scale
    assert not z["d_heatmap_d_box"].any() and not z["d_box_d_heat"].any()
    assert np.array_equal(box_only["box_2d_grad64"] != 0, box_only["touched"][:, None] & (box_only["box_2d_grad64"] != 0))
    # the scales are linear, and the fp32 result is the rounding of the float64 one
    both = loss_grad_ref.detection_loss_grad(z["heat"], z["box"], targets, stride=stride, heatmap_scale=2.0, box_scale=0.5, **settings)
    assert np.array_equal(both["heatmap_grad64"], 2.0 * heat_only["heatmap_grad64"]) and both["heatmap_grad"].dtype == np.float32
    assert np.array_equal(both["box_2d_grad"], both["box_2d_grad64"].astype(np.float32))


# ----------------------------------------------------------------------------- central differences of the value
EPS = 2.0 ** -10
FD_CASES = {
    "focal_giou": dict(box_loss="giou"),
    "quality_smooth": dict(heatmap_loss="quality", box_loss="smooth_l1", heatmap_target="ttfnet"),
    "l1_fixed": dict(box_loss="l1", heatmap_target="fixed", heatmap_target_params={"r": 2.0}),
    "iou": dict(box_loss="iou"),
    "diou_mult16": dict(box_loss="diou", box_multiplier=16.0),
    "ciou": dict(box_loss="ciou", heatmap_loss="quality"),
}


def fd_inputs(seed, settings, shape=(2, 3, 9, 11)):
    """Logits and box values at multiples of 2^-6 (x +- EPS d is exact in fp32, and so is the fp32 decode), boxes with centres inside the map."""
    rng = np.random.default_rng(seed)
    N, C, H, W = shape
    heat = (np.round(rng.normal(-2.0, 2.0, shape) * 64) / 64).astype(np.float32)
    box = (np.round(rng.uniform(0.25, 5.0, (N, 4, H, W)) * 64) / 64 / settings.get("box_multiplier", 1.0)).astype(np.float32)
    targets = []
    for n in range(N):
        m = 4
        wh = np.round(rng.uniform(6.0, 30.0, (m, 2)) * 8) / 8 + 1 / 16
        c = np.stack([rng.uniform(4, W * 4 - 5, m), rng.uniform(4, H * 4 - 5, m)], 1)
        targets.append((np.concatenate([np.round((c - wh / 2) * 8) / 8 + 1 / 32, wh], 1), rng.integers(0, C, m)))
    return heat, box, targets


@pytest.mark.parametrize("name", list(FD_CASES))
def test_restatement_against_central_differences_of_the_value(name):
    """(L(x + eps d) - L(x - eps d)) / (2 eps) against <grad, d>, d in {-1, 0, 1}: the truncation term is eps^2 / 6 of the third derivative along d,
    of the order of 1e-6 of the first for logits of a few units and boxes of a few pixels; the value itself carries 1e-16 / eps = 1e-13.  rtol 1e-4."""
    settings = FD_CASES[name]
    heat, box, targets = fd_inputs(sorted(FD_CASES).index(name) + 40, settings)
    C = heat.shape[1]
    away = loss_grad_ref.tie_distance(box, targets, C, **settings)
    assert away > 2 * EPS * 4, away                          # farther than the step moves a decoded corner (twice over)
    rng = np.random.default_rng(7)
    g = loss_grad_ref.detection_loss_grad(heat, box, targets, **settings)
    assert g["num_boxes"] > 20 and g["skipped"] == 0
    for key, arr, grad in (("heatmap", heat, g["heatmap_grad64"]), ("box_2d", box, g["box_2d_grad64"])):
        d = rng.integers(-1, 2, arr.shape).astype(np.float32)
        eps = EPS
        if key == "box_2d":
            d *= g["touched"][:, None]                       # (the other pixels do not move the value)
            eps = EPS / settings.get("box_multiplier", 1.0)  # a decoded corner moves by EPS * stride
        hi = loss_ref.detection_loss(*((arr + eps * d, box) if key == "heatmap" else (heat, arr + eps * d)), targets, **settings)[key]
        lo = loss_ref.detection_loss(*((arr - eps * d, box) if key == "heatmap" else (heat, arr - eps * d)), targets, **settings)[key]
        assert np.array_equal((arr + eps * d).astype(np.float32).astype(np.float64), arr.astype(np.float64) + eps * d.astype(np.float64))      # exact steps
        fd, dot = (hi - lo) / (2 * eps), float((grad * d).sum())
        print(name, key, "central difference", fd, "<grad, d>", dot, "relative", abs(fd - dot) / abs(dot))
        assert abs(dot) > 1e-3 * np.abs(grad * d).sum()      # the direction does not cancel the gradient away
        np.testing.assert_allclose(fd, dot, rtol=1e-4, atol=0)


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    for name in ("cnl_detection_loss_grad_workspace_bytes", "cnl_detection_loss_grad_f32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13
    assert lib.cnl_sizeof_params(4) == ctypes.sizeof(_lib.LossParams) == 72
    # the records (32 bytes per slot) and the two batch counts
    assert lib.cnl_detection_loss_grad_workspace_bytes(2, 3, 33, 70) == 2 * 3 * 32 + 16
    assert lib.cnl_detection_loss_grad_workspace_bytes(1, 1025, 4, 4) == 0 and lib.cnl_detection_loss_grad_workspace_bytes(1, 1, 0, 4) == 0
    assert lib.cnl_detection_loss_grad_workspace_bytes(1 << 16, 1, 4, 4) > 0 and lib.cnl_detection_loss_grad_workspace_bytes((1 << 16) + 1, 1, 4, 4) == 0


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    p = loss.loss_params(box_loss="giou")
    A = 1 << 20                                               # a well aligned address that is never read: every call below is refused before a launch

    def call(**kw):
        a = dict(heat=A, box=A, N=1, C=2, H=4, W=4, gt_boxes=A, gt_labels=A, gt_count=A, Gmax=1, p=ctypes.byref(p), scales=None, grad_heat=A, grad_box=A,
                 skipped=A, ws=A, ws_bytes=0)
        a.update(kw)
        return lib.cnl_detection_loss_grad_f32(a["heat"], 8, 1, 8, 2, a["box"], 64, 1, 16, 4, a["N"], a["C"], a["H"], a["W"], a["gt_boxes"], a["gt_labels"],
                                               a["gt_count"], a["Gmax"], a["p"], a["scales"], a["grad_heat"], 8, 1, 8, 2, a["grad_box"], 64, 1, 16, 4,
                                               a["skipped"], a["ws"], a["ws_bytes"], None)

    assert call(p=None) == _lib.CNL_E_BAD_ARG and "null params" in _lib.last_error()
    assert call(heat=None) == _lib.CNL_E_BAD_ARG and "needs the logits and the box map" in _lib.last_error()
    assert call(box=None) == _lib.CNL_E_BAD_ARG
    assert call(N=-1) == _lib.CNL_E_BAD_ARG and "N = -1" in _lib.last_error()
    assert call(C=0) == _lib.CNL_E_BAD_ARG and call(H=0) == _lib.CNL_E_BAD_ARG and call(W=(1 << 15) + 1) == _lib.CNL_E_BAD_ARG
    assert call(Gmax=1025) == _lib.CNL_E_BAD_ARG and "Gmax = 1025" in _lib.last_error()
    assert call(gt_count=None) == _lib.CNL_E_BAD_ARG and "null pointer" in _lib.last_error()
    assert call(skipped=None) == _lib.CNL_E_BAD_ARG and call(ws=None) == _lib.CNL_E_BAD_ARG
    assert call(scales=A + 4) == _lib.CNL_E_BAD_ARG and "8-byte aligned" in _lib.last_error()
    assert call(ws=A + 8) == _lib.CNL_E_BAD_ARG and call(grad_heat=A + 2) == _lib.CNL_E_BAD_ARG and call(gt_boxes=A + 4) == _lib.CNL_E_BAD_ARG
    assert call(ws_bytes=32 + 15) == _lib.CNL_E_WORKSPACE and "48 needed" in _lib.last_error()
    assert call(N=0, gt_boxes=None, ws=None) == 0                      # an empty batch: nothing to do
    p.box_loss = 9
    assert call() == _lib.CNL_E_BAD_ARG and "box_loss = 9" in _lib.last_error()
    p.box_loss, p.stride = 3, 0.0
    assert call() == _lib.CNL_E_BAD_ARG and "stride" in _lib.last_error()


# ----------------------------------------------------------------------------- the Python layer
def _maps(N=2, C=3, H=4, W=5):
    return torch.zeros(N, C, H, W), torch.zeros(N, 4, H, W)


def _targets(N=2):
    return [{"boxes": [[0.0, 0.0, 4.0, 4.0]], "labels": [0]} for _ in range(N)]


@pytest.mark.parametrize("kwargs, match", [
    (dict(box_loss="L2Loss"), "box_loss must be one of"),
    (dict(stride=0), "stride must be a finite positive number"),
    (dict(want="heatmap"), "want must be a non-empty tuple"),
    (dict(want=()), "want must be a non-empty tuple"),
    (dict(want=("heatmap", "reid")), "want must be a non-empty tuple"),
    (dict(want=("box_2d", "box_2d")), "want must be a non-empty tuple"),
    (dict(heatmap_scale="1"), "heatmap_scale must be a finite number"),
    (dict(box_scale=float("inf")), "box_scale must be a finite number"),
    (dict(box_scale=torch.ones(2, dtype=torch.float64)), "box_scale as a tensor must be float64 with one element"),
    (dict(heatmap_scale=torch.ones(())), "heatmap_scale as a tensor must be float64 with one element"),
])
def test_detection_loss_grad_checks_its_arguments_before_any_launch(kwargs, match):
    heat, box = _maps()
    with pytest.raises(ValueError, match=match):
        cl.detection_loss_grad(heat, box, _targets(), **kwargs)


def test_maps_are_checked_and_there_is_no_cpu_fallback():
    heat, box = _maps()
    with pytest.raises(ValueError, match="heatmap must be a float32 tensor"):
        cl.detection_loss_grad(heat.half(), box, _targets())
    with pytest.raises(ValueError, match="box_2d must be a float32 tensor"):
        cl.detection_loss_grad(heat, box.double(), _targets())
    with pytest.raises(ValueError, match=r"needs box_2d \[2, 4, 4, 5\]"):
        cl.detection_loss_grad(heat, box[:, :, :2], _targets())
    with pytest.raises(RuntimeError, match="HIP devices only"):
        cl.detection_loss_grad(heat, box, _targets())
    criterion = cl.DetectionLoss(box_loss="giou")
    with pytest.raises(ValueError, match="outputs must be the dict of get_encoded_outputs"):
        criterion((heat, box), _targets())
    with pytest.raises(RuntimeError, match="HIP devices only"):               # with and without a graph: no CPU fallback
        criterion({"heatmap": heat.clone().requires_grad_(), "box_2d": box}, _targets())
    with pytest.raises(RuntimeError, match="HIP devices only"):
        criterion({"heatmap": heat, "box_2d": box}, _targets())
    with pytest.raises(ValueError, match="heatmap must be a float32 tensor"):
        criterion({"heatmap": heat.double().requires_grad_(), "box_2d": box}, _targets())
    with pytest.raises(ValueError, match="box_loss must be one of"):
        cl.DetectionLoss(box_loss="huber")


def test_exports_and_the_model_criterion():
    assert "DetectionLoss" in cl.__all__ and "detection_loss_grad" in cl.__all__
    assert cl.DetectionLoss is loss.DetectionLoss and cl.detection_loss_grad is loss.detection_loss_grad
    assert issubclass(cl.DetectionLoss, torch.nn.Module)
    assert cl.DetectionLoss(box_loss="l1", return_targets=True).settings == {"box_loss": "l1"}
    cfg = {"model": {"backbone": {"name": "resnet18"}, "neck": {"name": "fpn"}, "box_multiplier": 16.0, "box_loss": "L1Loss", "box_loss_weight": 0.1,
                     "output_heads": {"heatmap": {"num_classes": 2, "target_method": "ttfnet"}, "box_2d": {"loss_function": "giou", "loss_weight": 5}}}}
    model = cl.build_centernet(cfg)
    criterion = model.criterion()
    assert isinstance(criterion, cl.DetectionLoss)
    assert criterion.settings == model.loss_meter().settings == model._loss_kwargs(None)
    assert criterion.settings["box_multiplier"] == 16.0 and criterion.settings["box_loss"] == "L1Loss" and criterion.settings["stride"] == model.stride
