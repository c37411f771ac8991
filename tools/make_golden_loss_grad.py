"""Writes tests/golden/grad_loss_*.npz (not loss_grad_*: tests/test_loss_host.py reads every loss_*.npz as a forward fixture):
the gradients torch's autograd gives for the reference's CenterNet.compute_loss on seeded float64 head
outputs (needs the reference tree, like tools/make_golden_loss.py and the generators under oracle/; the tests read only the recorded files).

    python tools/make_golden_loss_grad.py

Cases: the families of tools/make_golden_loss.py at its small shapes (every target method, both heatmap losses, all six box losses, box_log,
multiplier 16, edges, radius 0), and `ties*` cases that plant every non-differentiable point the rule of include/centernet_gfx950.h names: a decoded
corner that EQUALS the target's (maximum / minimum ties), an intersection of width exactly 0, box values of exactly 0 and below 0 (the clamp), l1
differences of exactly 0, smooth_l1 differences of exactly 1, and sigmoid(x) == t exactly under the quality loss.

Every file holds the inputs, the settings and the four gradients, float64: d heatmap / d heat, d heatmap / d box_2d (zeros), d box_2d / d heat (zeros),
d box_2d / d box_2d, where "heatmap" and "box_2d" are compute_loss's two normalised losses.  The restatement tests/loss_grad_ref.py is compared with
them before anything is written: the worst max|restatement - reference| / max|reference| over all cases and tensors is printed and stored in every
file ("tol64"); tests/test_loss_grad_host.py allows four times that.  (The reference's float64 run decodes the boxes in float64, the rule in fp32 as
the forward does: that difference, an fp32 ulp of a box corner, is what tol64 measures on the box gradients.)"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_import  # noqa: E402
import loss_grad_ref  # noqa: E402
import make_golden_loss as base  # noqa: E402

STRIDE = base.STRIDE
LARGE = ("wide", "ttf_quality")              # the 33 x 70 cases of the forward's generator: the GPU tests cover that shape against the restatement
GRADS = ("d_heatmap_d_heat", "d_heatmap_d_box", "d_box_d_heat", "d_box_d_box")


def ties_case(box_loss, deltas, heatmap_loss="cornernet_focal", seed=20):
    """One image, 2 classes, 12 x 16 map.  Box A: at each of its nine samples the decoded box is the target + deltas (input pixels, exact in fp32).
    Box B: its samples hold box values of exactly 0 and below 0.  Box C: an ordinary box of B's class."""
    rng = np.random.default_rng(seed)
    C, H, W = 2, 12, 16
    heat = rng.normal(-2.0, 2.0, (1, C, H, W)).astype(np.float32)
    box = rng.uniform(0.5, 6.0, (1, 4, H, W)).astype(np.float32)
    boxes = np.array([[10.0, 6.0, 28.0, 24.0],           # A: centre (6, 4.5 -> 4)
                      [40.0, 8.0, 8.0, 8.0],             # B: centre (11, 3)
                      [8.0, 30.0, 16.0, 8.0]])           # C: centre (4, 8.5 -> 8)
    labels = np.array([0, 1, 1], np.int64)
    t = np.array([10.0, 6.0, 38.0, 30.0])
    for x in (5, 6, 7):
        for y in (3, 4, 5):
            p = t + np.asarray(deltas, np.float64)
            v = np.array([(x + 0.5) - p[0] / STRIDE, (y + 0.5) - p[1] / STRIDE, p[2] / STRIDE - (x + 0.5), p[3] / STRIDE - (y + 0.5)])
            assert (v >= 0).all() and np.array_equal(v.astype(np.float32).astype(np.float64), v)
            box[0, :, y, x] = v
    box[0, :, 3, 11] = [0.0, 1.0, -0.5, 2.0]             # B's centre: the clamp at exactly 0 and below it
    box[0, :, 2, 10] = [0.0, 0.0, 1.0, 2.0]
    box[0, :, 4, 12] = [-1.0, -0.0, 0.0, 1.5]
    # the quality loss: sigmoid(x) == t exactly at a peak (t = 1, x = +800) and far from every box (t = 0, x = -800)
    heat[0, 0, 4, 6] = 800.0
    heat[0, 1, 11, 15] = -800.0
    heat[0, 0, 11, 0] = -800.0
    settings = dict(box_loss=box_loss, heatmap_loss=heatmap_loss, heatmap_target="fixed", heatmap_target_params={"r": 2.0})
    return {"shape": (1, C, H, W), "targets": [(boxes, labels)], "heat": heat, "box": box, "settings": settings}


def zero_width_case(box_loss, seed=21):
    """One box; at one of its samples the decoded x1 equals the target's x2 (intersection width exactly 0: the clamp passes the gradient), at two others
    the decoded y1 equals the target's y2 (height exactly 0)."""
    rng = np.random.default_rng(seed)
    C, H, W = 1, 8, 8
    heat = rng.normal(-2.0, 2.0, (1, C, H, W)).astype(np.float32)
    box = rng.uniform(0.5, 3.0, (1, 4, H, W)).astype(np.float32)
    boxes = np.array([[16.0, 12.0, 8.0, 8.0]])           # target (16, 12, 24, 20), centre (5, 4)
    box[0, :, 4, 6] = [0.5, 1.0, 1.0, 1.0]               # sample (6, 4): x1 = 24 == the target's x2: width 0, height 6
    box[0, :, 5, 4] = [1.5, 0.5, 0.0, 0.5]               # sample (4, 5): y1 = 20 == the target's y2: height 0, width 2 (x2 = 18 from a box value of 0)
    box[0, :, 5, 6] = [1.0, 0.5, 1.0, 1.5]               # sample (6, 5): y1 = 20: height 0, width 2
    settings = dict(box_loss=box_loss, heatmap_target="fixed", heatmap_target_params={"r": 1.0})
    return {"shape": (1, C, H, W), "targets": [(boxes, np.array([0], np.int64))], "heat": heat, "box": box, "settings": settings}


def cases():
    out = {k: v for k, v in base.cases().items() if k not in LARGE}
    out["ties"] = ties_case("l1", (0.0, 0.5, -0.25, 0.0), heatmap_loss="quality")
    out["ties_smooth"] = ties_case("smooth_l1", (1.0, -1.0, 0.5, 2.0))
    for kind in ("iou", "giou", "diou", "ciou"):
        out[f"ties_{kind}"] = ties_case(kind, (0.0, 1.0, 0.0, -2.0))
        out[f"ties_zero_{kind}"] = zero_width_case(kind)
    return out


def reference_grads(ref, case):
    """-> the four gradients (GRADS order) of the reference's float64 run, numpy float64"""
    CenterNet, heatmap_losses, box_losses, radius = ref
    st = case["settings"]
    fake = SimpleNamespace(stride=STRIDE, device=torch.device("cpu"),
                           hparams=SimpleNamespace(box_log=st.get("box_log", False), box_multiplier=st.get("box_multiplier", 1.0),
                                                   heatmap_loss_weight=st.get("heatmap_loss_weight", 1.0), box_loss_weight=st.get("box_loss_weight", 1.0)),
                           heatmap_loss=getattr(heatmap_losses, base.GEN_B[st.get("heatmap_loss", "cornernet_focal")])(reduction="sum"),
                           box_loss=getattr(box_losses, base.GEN_B[st.get("box_loss", "giou")])(reduction="sum"),
                           heatmap_radius=radius[st.get("heatmap_target", "cornernet")](**(st.get("heatmap_target_params") or {})))
    targets = [{"boxes": [[float(v) for v in b] for b in boxes], "labels": [int(v) for v in labels]} for boxes, labels in case["targets"]]
    heat = torch.from_numpy(case["heat"]).to(torch.float64).requires_grad_(True)
    box = torch.from_numpy(case["box"]).to(torch.float64).requires_grad_(True)
    losses = CenterNet.compute_loss(fake, {"heatmap": heat, "box_2d": box}, targets)
    out = []
    for key in ("heatmap", "box_2d"):
        if losses[key].requires_grad:
            grads = torch.autograd.grad(losses[key], [heat, box], retain_graph=True, allow_unused=True)
        else:
            grads = (None, None)
        out += [np.zeros(t.shape) if g is None else g.numpy().copy() for g, t in zip(grads, (heat, box))]
    return out


def main():
    CenterNet = _ref_import.import_reference_centernet()
    mod = sys.modules["centernet_lightning.models.centernet"]
    ref = (CenterNet, mod.heatmap_losses, mod.box_losses, mod._heatmap_targets)
    out_dir = os.path.join(ROOT, "tests", "golden")
    files, worst = {}, 0.0
    for name, case in cases().items():
        st = case["settings"]
        grads = reference_grads(ref, case)
        assert not grads[1].any() and not grads[2].any(), name                       # the cross terms
        ours_h = loss_grad_ref.detection_loss_grad(case["heat"], case["box"], case["targets"], stride=STRIDE, heatmap_scale=1.0, box_scale=0.0, **st)
        ours_b = loss_grad_ref.detection_loss_grad(case["heat"], case["box"], case["targets"], stride=STRIDE, heatmap_scale=0.0, box_scale=1.0, **st)
        mine = [ours_h["heatmap_grad64"], ours_h["box_2d_grad64"], ours_b["heatmap_grad64"], ours_b["box_2d_grad64"]]
        dev = np.zeros(4)
        for i, (m, r) in enumerate(zip(mine, grads)):
            assert np.isfinite(r).all() and np.isfinite(m).all(), (name, GRADS[i])
            if r.any():
                dev[i] = np.abs(m - r).max() / np.abs(r).max()
            else:
                assert not m.any(), (name, GRADS[i])
        assert np.array_equal(grads[3] != 0, ours_b["touched"][:, None] & (grads[3] != 0)), name      # nothing outside the sampled pixels
        worst = max(worst, float(dev.max()))
        N, C, H, W = case["shape"]
        print(f"{name:16s} {case['shape']} boxes {[len(l) for _, l in case['targets']]} max|d heat| {np.abs(grads[0]).max():.3e} max|d box| "
              f"{np.abs(grads[3]).max():.3e} dev heat {dev[0]:.3e} dev box {dev[3]:.3e}")
        G = max([1] + [len(l) for _, l in case["targets"]])
        boxes, labels = np.full((N, G, 4), np.nan), np.full((N, G), -1, np.int64)
        count = np.array([len(l) for _, l in case["targets"]], np.int32)
        for n, (b, l) in enumerate(case["targets"]):
            boxes[n, :len(l)], labels[n, :len(l)] = b, l
        files[name] = dict(heat=case["heat"], box=case["box"], boxes=boxes, labels=labels, count=count, settings=json.dumps(st), stride=STRIDE, dev=dev,
                           **dict(zip(GRADS, grads)))
    print(f"worst relative deviation of the restatement from the float64 reference: {worst:.3e}")
    limit = max(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir) if f.startswith("loss_"))
    for name, arrays in files.items():
        path = os.path.join(out_dir, f"grad_loss_{name}.npz")
        np.savez_compressed(path, tol64=worst, **arrays)
        size = os.path.getsize(path)
        assert size <= limit, (path, size, limit)
        print("wrote", os.path.relpath(path, ROOT), size, "bytes")


if __name__ == "__main__":
    main()
