"""Writes tests/golden/loss_*.npz: the reference's CenterNet.compute_loss and update_heatmap on seeded inputs (needs the reference tree, like the
generators under oracle/; the tests read only the recorded files).

    python tools/make_golden_loss.py

The reference's loss modules and radius classes hang on a SimpleNamespace that stands in for the Lightning module.  Every case is run twice, with
fp32 and with float64 head outputs, and compared with the restatement tests/loss_ref.py:
  * the target map: fp32 bits, at most 1 ulp apart in at most 1 in 10^4 rendered elements (torch's fp32 exp against numpy's float64 exp) — ASSERTED
    here, before anything is written;
  * record integers (centres, sample indices, counts): equal — asserted here;
  * the three losses: the worst relative deviation of the restatement from the float64 run and from the fp32 run over all cases is printed and
    stored in every file ("tol64", "tol32"); tests/test_loss_host.py allows four times that.
"""
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_import  # noqa: E402
import loss_ref  # noqa: E402

GEN_B = {"l1": "L1Loss", "smooth_l1": "SmoothL1Loss", "iou": "IoULoss", "giou": "GIoULoss", "diou": "DIoULoss", "ciou": "CIoULoss",
         "cornernet_focal": "CornerNetFocalLoss", "quality": "QualityFocalLoss"}
STRIDE = 4


def random_boxes(rng, m, H, W, max_size=48.0):
    """m boxes x y w h in input pixels (multiples of 1/8) whose centres fall inside the map."""
    wh = np.round(rng.uniform(2.0, max_size, (m, 2)) * 8) / 8
    c = np.stack([rng.uniform(0, W * STRIDE - 1, m), rng.uniform(0, H * STRIDE - 1, m)], 1)
    xy = np.round((c - wh / 2) * 8) / 8
    return np.concatenate([xy, wh], 1)


def cases():
    """name -> dict(shape, targets [(boxes, labels)], settings)"""
    out = {}

    def add(name, seed, shape, counts, special=None, **settings):
        rng = np.random.default_rng(seed)
        N, C, H, W = shape
        targets = []
        for n in range(N):
            b = random_boxes(rng, counts[n], H, W)
            lab = rng.integers(0, C, counts[n])
            if special and n == 0:
                sb, sl = special(H, W, C)
                b, lab = np.concatenate([np.asarray(sb, np.float64).reshape(-1, 4), b]), np.concatenate([np.asarray(sl, np.int64), lab])
            targets.append((b, lab.astype(np.int64)))
        heat = rng.normal(-2.0, 2.0, shape).astype(np.float32)
        box = (rng.uniform(-1.0, 1.5, (N, 4, H, W)) if settings.get("box_log") else
               rng.uniform(-0.5, 6.0, (N, 4, H, W)) / settings.get("box_multiplier", 1.0)).astype(np.float32)
        out[name] = {"shape": shape, "targets": targets, "heat": heat, "box": box, "settings": settings}

    def on_edges(H, W, C):
        s = STRIDE
        return ([[W * s - 8, 10, 16, 12],            # cx == W
                 [20, H * s - 6, 8, 12],              # cy == H
                 [-4, -6, 8, 12],                     # centre at (0, 0)
                 [W * s - 4, H * s - 4, 8, 8],        # cx == W and cy == H
                 [24, 20, 24, 16], [28, 24, 24, 16],  # two same-class boxes whose Gaussians overlap
                 [0, 0, W * s * 6, H * s * 6]],       # (with ttfnet) a radius larger than the map; its centre is outside: see "huge"
                [0, 1, 0, 1, 1, 1, 0])

    add("one", 1, (1, 1, 1, 1), [0], special=lambda H, W, C: ([[0, 0, 2, 2], [2, 2, 4, 4]], [0, 0]), box_loss="l1")
    add("tiny", 2, (1, 2, 3, 5), [3], heatmap_target="ttfnet", heatmap_loss="quality", box_loss="l1")
    add("mid", 3, (2, 3, 16, 20), [9, 0], heatmap_target="fixed", box_loss="smooth_l1", heatmap_loss_weight=0.5, box_loss_weight=0.1)
    add("wide", 4, (2, 5, 33, 70), [130, 40], box_loss="giou", box_loss_weight=5.0)
    add("edges", 5, (1, 2, 16, 20), [4], special=lambda H, W, C: tuple(v[:6] for v in on_edges(H, W, C)), box_loss="iou")
    # radii (6, 4) on a 3 x 5 map.  (On a large map such a window holds hundreds of distinct exponents, and torch's fp32 exp differs from the
    # correctly rounded value in about 2 % of them: the 1-in-10^4 cap below can only be met where a window holds few distinct ones.)
    add("huge", 6, (1, 2, 3, 5), [1], special=lambda H, W, C: ([[-20, -14, 60, 40], [0, 0, 20, 12]], [0, 1]), heatmap_target="ttfnet",
        heatmap_target_params={"alpha": 0.8}, box_loss="giou")
    add("mult16", 7, (1, 3, 16, 20), [12], box_multiplier=16.0, box_loss="diou", heatmap_target_params={"min_overlap": 0.5})
    add("log", 8, (1, 2, 16, 20), [10], box_log=True, box_loss="ciou", heatmap_loss="quality")
    add("ttf_quality", 9, (2, 5, 33, 70), [0, 20], heatmap_target="ttfnet", heatmap_loss="quality", box_loss="l1")
    add("fixed3", 10, (1, 1, 3, 5), [2], heatmap_target="fixed", heatmap_target_params={"r": 3.0}, box_loss="smooth_l1")
    add("radius0", 11, (1, 2, 16, 20), [6], heatmap_target="fixed", heatmap_target_params={"r": 0.0}, box_loss="ciou")
    return out


def reference_run(ref, case, dtype):
    """-> (target map [N,C,H,W] as the reference renders it in `dtype`, losses [3] in `dtype`, num_dets, sample indices per image)"""
    CenterNet, heatmap_losses, box_losses, radius = ref
    st = case["settings"]
    method = st.get("heatmap_target", "cornernet")
    fake = SimpleNamespace(stride=STRIDE, device=torch.device("cpu"),
                           hparams=SimpleNamespace(box_log=st.get("box_log", False), box_multiplier=st.get("box_multiplier", 1.0),
                                                   heatmap_loss_weight=st.get("heatmap_loss_weight", 1.0), box_loss_weight=st.get("box_loss_weight", 1.0)),
                           heatmap_loss=getattr(heatmap_losses, GEN_B[st.get("heatmap_loss", "cornernet_focal")])(reduction="sum"),
                           box_loss=getattr(box_losses, GEN_B[st.get("box_loss", "giou")])(reduction="sum"),
                           heatmap_radius=radius[method](**(st.get("heatmap_target_params") or {})))
    targets = [{"boxes": [[float(v) for v in b] for b in boxes], "labels": [int(v) for v in labels]} for boxes, labels in case["targets"]]
    outputs = {"heatmap": torch.from_numpy(case["heat"]).to(dtype), "box_2d": torch.from_numpy(case["box"]).to(dtype)}
    losses = CenterNet.compute_loss(fake, outputs, targets)
    # the target map, as compute_loss builds it (centernet.py:134-146)
    tmap = torch.zeros_like(outputs["heatmap"])
    for i, inst in enumerate(targets):
        if len(inst["labels"]) == 0:
            continue
        boxes = np.array(inst["boxes"]) / STRIDE
        centers = (boxes[..., :2] + boxes[..., 2:] / 2).round().astype(int)
        radii = [fake.heatmap_radius(w, h) for w, h in boxes[..., 2:]]
        CenterNet.update_heatmap(tmap[i], centers, radii, inst["labels"])
    return tmap.numpy(), np.array([losses[k].item() for k in ("heatmap", "box_2d", "total")], dtype=np.float64)


def ulp_apart(a, b):
    """fp32 arrays -> |distance in units in the last place| (both non-negative floats)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def main():
    CenterNet = _ref_import.import_reference_centernet()
    mod = sys.modules["centernet_lightning.models.centernet"]
    ref = (CenterNet, mod.heatmap_losses, mod.box_losses, mod._heatmap_targets)
    out_dir = os.path.join(ROOT, "tests", "golden")
    files, worst32, worst64 = {}, np.zeros(3), np.zeros(3)
    for name, case in cases().items():
        st = case["settings"]
        ours = loss_ref.detection_loss(case["heat"], case["box"], case["targets"], stride=STRIDE, **st)
        map32, loss32 = reference_run(ref, case, torch.float32)
        map64, loss64 = reference_run(ref, case, torch.float64)
        assert np.array_equal(map32.astype(np.float64), map64), name               # the Gaussian is fp32 in both runs
        # target map: bits, 1 ulp in at most 1 in 10^4 rendered elements
        rendered = max(int(np.count_nonzero(map32)), 1)
        apart = ulp_apart(ours["targets"], map32)
        differ = int(np.count_nonzero(apart))
        assert apart.max(initial=0) <= 1 and differ * 10 ** 4 <= rendered, (name, int(apart.max(initial=0)), differ, rendered)
        assert np.array_equal(ours["targets"] == 0, map32 == 0), name
        # integers: counts against the reference's normalisers (recovered from its sums is not possible: compare through the loop restated here)
        N, C, H, W = case["shape"]
        for n, (boxes, labels) in enumerate(case["targets"]):
            if len(labels) == 0:
                assert ours["per_image"][n, 2] == 0 and ours["per_image"][n, 3] == 0
                continue
            b = np.array([[float(v) for v in bb] for bb in boxes]) / STRIDE
            centers = (b[..., :2] + b[..., 2:] / 2).round().astype(int)
            idx = []
            for (cx, cy) in centers:
                cxs = [d for d in [cx - 1, cx, cx + 1] if 0 <= d <= W - 1]
                cys = [d for d in [cy - 1, cy, cy + 1] if 0 <= d <= H - 1]
                idx += [int(y * W + x) for x, y in itertools.product(cxs, cys)]
            assert [(r["cx"], r["cy"]) for r in ours["records"][n]] == [tuple(int(v) for v in c) for c in centers], name
            assert ours["samples"][n] == idx, name
            assert ours["per_image"][n, 2] == len(labels) and ours["per_image"][n, 3] == len(idx), name
        assert ours["skipped"] == 0, name
        mine = np.array([ours["heatmap"], ours["box_2d"], ours["total"]])
        dev32, dev64 = np.abs(mine - loss32) / np.maximum(np.abs(loss32), 1e-300), np.abs(mine - loss64) / np.maximum(np.abs(loss64), 1e-300)
        dev32[loss32 == mine], dev64[loss64 == mine] = 0, 0
        worst32, worst64 = np.maximum(worst32, dev32), np.maximum(worst64, dev64)
        print(f"{name:12s} {case['shape']} boxes {[len(l) for _, l in case['targets']]} rendered {rendered} map elements differing {differ} "
              f"dev fp32 {dev32.max():.3e} dev f64 {dev64.max():.3e}")
        G = max([1] + [len(l) for _, l in case["targets"]])
        boxes, labels = np.full((N, G, 4), np.nan), np.full((N, G), -1, np.int64)
        count = np.array([len(l) for _, l in case["targets"]], np.int32)
        for n, (b, l) in enumerate(case["targets"]):
            boxes[n, :len(l)], labels[n, :len(l)] = b, l
        files[name] = dict(heat=case["heat"], box=case["box"], boxes=boxes, labels=labels, count=count, settings=json.dumps(st), stride=STRIDE,
                           target_map=map32, loss32=loss32.astype(np.float32), loss64=loss64, dev32=dev32, dev64=dev64,
                           num_dets=ours["per_image"][:, 2].astype(np.int64), num_boxes=ours["per_image"][:, 3].astype(np.int64))
    tol32, tol64 = float(worst32.max()), float(worst64.max())
    print(f"worst relative deviation of the restatement: fp32 golden {tol32:.3e}, float64 golden {tol64:.3e}")
    for name, arrays in files.items():
        path = os.path.join(out_dir, f"loss_{name}.npz")
        np.savez_compressed(path, tol32=tol32, tol64=tol64, **arrays)
        print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
