"""Writes tests/golden/reid_loss_*.npz: the value, the gradients torch's autograd gives and the BatchNorm buffers after the step for the reference's
EmbeddingHead.compute_loss (models/fairmot.py:34-61) on seeded float64 copies of fp32 inputs (needs the reference tree, like tools/make_golden_loss.py
and the generators under oracle/; the tests read only the recorded files).

    python tools/make_golden_reid_loss.py

The reference method is called unbound on a SimpleNamespace that carries `classifier` (the reference's nn.Sequential, in float64) and `loss_function`
(nn.CrossEntropyLoss(reduction="none")), in the manner of oracle/_ref_import.make_fake_self.  Its targets are the reference's own form: centres
normalised by the input size, zero-padded to Gmax, with a mask.

Cases: full masks; a padded batch (padded_rows=True: the zero boxes enter the BatchNorm statistics at cell (0, 0)); two boxes in one cell; a box in cell
(0, 0) beside padded rows; eval mode.  Every file holds the inputs (reid fp32, boxes x y w h in input pixels with NaN beyond the count, ids, count, the
seven classifier tensors fp32), the settings, the loss, the six gradients (the map and the five trainable tensors) and the running statistics after the
step, float64.  The restatement tests/reid_loss_ref.py is compared with them before anything is written: the worst max|restatement - reference| /
max|reference| over all cases and tensors is printed and stored in every file ("tol64"); tests/test_reid_loss_host.py allows four times that."""
import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_import  # noqa: E402
import reid_loss_ref  # noqa: E402

STRIDE = 4
D, K, H, W = 16, 23, 6, 8


def boxes_at(centres, sizes):
    c, s = np.asarray(centres, np.float64) * STRIDE, np.asarray(sizes, np.float64) * STRIDE
    return np.concatenate([c - s / 2, s], 1)


def make(seed, per_image, training=True, padded_rows=False):
    """per_image: a list of (centres in map pixels, sizes in map pixels) per image"""
    rng = np.random.default_rng(seed)
    N, G = len(per_image), max(len(c) for c, _ in per_image)
    boxes, ids = np.full((N, G, 4), np.nan), np.full((N, G), -7, np.int64)
    count = np.array([len(c) for c, _ in per_image], np.int32)
    for n, (c, s) in enumerate(per_image):
        if len(c):
            boxes[n, :len(c)] = boxes_at(c, s)
            ids[n, :len(c)] = rng.choice(K, len(c), replace=False)
    cls = dict(W1=rng.normal(0, 1 / np.sqrt(D), (D, D)), gamma=rng.uniform(0.5, 1.5, D), beta=rng.normal(0, 0.3, D), running_mean=rng.normal(0, 0.2, D),
               running_var=rng.uniform(0.5, 1.5, D), W2=rng.normal(0, 2 / np.sqrt(D), (K, D)), b2=rng.normal(0, 0.5, K))
    return dict(reid=rng.normal(0, 1, (N, D, H, W)).astype(np.float32), boxes=boxes, ids=ids, count=count, cls={k: v.astype(np.float32) for k, v in cls.items()},
                settings=dict(training=training, padded_rows=padded_rows, center="trunc", stride=STRIDE, bn_eps=1e-5, momentum=0.1))


def cases():
    s2, s3 = [[2, 2], [1, 3]], [[2, 2], [1, 3], [3, 1]]
    return {
        "full": make(1, [([[1.3, 2.6], [6.2, 0.4], [4.5, 4.5]], s3), ([[7.7, 5.2], [0.6, 3.1], [3.3, 1.8]], s3)]),
        "padded": make(2, [([[1.3, 2.6], [6.2, 0.4], [4.5, 4.5]], s3), ([], []), ([[5.1, 3.3], [2.8, 5.9]], s2)], padded_rows=True),
        "shared_cell": make(3, [([[3.2, 2.1], [3.7, 2.8], [6.4, 4.4]], s3), ([[3.2, 2.1], [0.2, 5.5], [7.9, 0.1]], s3)]),
        "origin": make(4, [([[0.4, 0.7], [5.5, 2.5]], s2), ([[2.2, 4.4]], [[2, 2]]), ([], [])], padded_rows=True),
        "eval": make(5, [([[1.3, 2.6], [6.2, 0.4], [4.5, 4.5]], s3), ([[5.1, 3.3]], [[1, 1]])], training=False, padded_rows=True),
    }


def reference(EmbeddingHead, case):
    """-> (loss, the six gradients by reid_loss_ref.GRADS, running_mean, running_var after the call), float64"""
    cls, st = case["cls"], case["settings"]
    seq = nn.Sequential(nn.Linear(D, D, bias=False), nn.BatchNorm1d(D, eps=st["bn_eps"], momentum=st["momentum"]), nn.ReLU(inplace=True), nn.Linear(D, K)).double()
    with torch.no_grad():
        for t, k in ((seq[0].weight, "W1"), (seq[1].weight, "gamma"), (seq[1].bias, "beta"), (seq[1].running_mean, "running_mean"),
                     (seq[1].running_var, "running_var"), (seq[3].weight, "W2"), (seq[3].bias, "b2")):
            t.copy_(torch.from_numpy(cls[k].astype(np.float64)))
    seq.train(st["training"])
    fake = SimpleNamespace(classifier=seq, loss_function=nn.CrossEntropyLoss(reduction="none"))
    N, G = case["ids"].shape
    mask = (np.arange(G)[None, :] < case["count"][:, None])
    b = np.where(mask[..., None], case["boxes"], 0.0)
    cxcywh = np.stack([(b[..., 0] + b[..., 2] / 2) / (W * STRIDE), (b[..., 1] + b[..., 3] / 2) / (H * STRIDE), b[..., 2] / (W * STRIDE), b[..., 3] / (H * STRIDE)], -1)
    target = {"bboxes": torch.from_numpy(cxcywh), "ids": torch.from_numpy(np.where(mask, case["ids"], 0)), "mask": torch.from_numpy(mask.astype(np.float64))}
    reid = torch.from_numpy(case["reid"].astype(np.float64)).requires_grad_(True)
    loss = EmbeddingHead.compute_loss(fake, {"reid": reid}, target)
    loss.backward()
    grads = [reid.grad, seq[0].weight.grad, seq[1].weight.grad, seq[1].bias.grad, seq[3].weight.grad, seq[3].bias.grad]
    return float(loss.detach()), [g.numpy().copy() for g in grads], seq[1].running_mean.numpy().copy(), seq[1].running_var.numpy().copy()


def main():
    _ref_import.import_reference_centernet()                 # the stubs for the reference's absent third-party dependencies
    # fairmot.py imports the tracker (filterpy) and names that its own tree no longer defines: one base class in models/meta.py, four helpers in utils,
    # one in eval.  None of them is executed by compute_loss; placeholders, as for the stubs of oracle/_ref_import.py.
    _ref_import._stub("filterpy").kalman = _ref_import._stub("filterpy.kalman")
    absent = {"centernet_lightning.models.meta": {"BaseHead": nn.Module},
              "centernet_lightning.utils": dict.fromkeys(("box_iou_distance_matrix", "box_giou_distance_matrix", "load_config", "convert_box_format"), _ref_import._Any),
              "centernet_lightning.eval": {"evaluate_mot_tracking_sequence": _ref_import._Any}}
    for module, names in absent.items():
        mod = importlib.import_module(module)
        for name, placeholder in names.items():
            if not hasattr(mod, name):
                setattr(mod, name, placeholder)
    EmbeddingHead = importlib.import_module("centernet_lightning.models.fairmot").EmbeddingHead
    out_dir = os.path.join(ROOT, "tests", "golden")
    files, worst = {}, 0.0
    for name, case in cases().items():
        st = case["settings"]
        loss, grads, mean, var = reference(EmbeddingHead, case)
        args = (case["reid"], case["boxes"], case["ids"], case["count"], case["cls"])
        mine = reid_loss_ref.reid_loss(*args, **st)
        mine_g = reid_loss_ref.reid_loss_grad(*args, **st)
        pairs = [(np.array(mine["reid"]), np.array(loss)), (mine["running_mean64"], mean), (mine["running_var64"], var)] + \
            [(mine_g[k], g) for k, g in zip(reid_loss_ref.GRADS, grads)]
        dev = []
        for m, r in pairs:
            assert np.isfinite(r).all() and np.isfinite(m).all() and np.abs(r).max() > 0, name
            dev.append(float(np.abs(m - r).max() / np.abs(r).max()))
        assert np.array_equal(grads[0].any(axis=1), mine_g["read"] & grads[0].any(axis=1)), name      # nothing outside the cells some row reads
        worst = max(worst, max(dev))
        print(f"{name:12s} rows {mine['num_rows']} loss {loss:.6f} deviations {' '.join(f'{d:.1e}' for d in dev)}")
        files[name] = dict(reid=case["reid"], boxes=case["boxes"], ids=case["ids"], count=case["count"], settings=json.dumps(st), loss=np.array(loss),
                           running_mean_after=mean, running_var_after=var, **case["cls"], **{"d_" + k: g for k, g in zip(reid_loss_ref.GRADS, grads)})
    print(f"worst relative deviation of the restatement from the float64 reference: {worst:.3e}")
    for name, arrays in files.items():
        path = os.path.join(out_dir, f"reid_loss_{name}.npz")
        np.savez_compressed(path, tol64=worst, **arrays)
        print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
