"""Times CocoEvaluator (csrc/coco_eval.hip) on a synthetic COCO-val-sized epoch and compares it with the numpy restatement of the
same rule (tests/coco_eval_ref.py) run on the host over the same data.  pycocotools is not available to time; the restatement is a
plain-Python walk and far slower than pycocotools' C matcher, so its time is an upper bound on "host evaluation", not a measurement of it.

    python tools/coco_eval_bench.py [--images 5000] [--k 100] [--classes 80] [--batch 32] [--ref-images 200] [--out profiles/coco_eval_bench.txt]

5,000 images, k = 100 detections, 80 classes, about 7 ground truths per image.  update() is timed per batch of 32 (device time between
events, and host wall time of the call: it does not synchronise); get_metrics() is timed whole, download included.  The restatement runs
over the first --ref-images images only (its time scales linearly; the tool says so) and the evaluator over the same subset must agree
with it bit for bit, or the tool fails.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import centernet_lightning_amd as cl  # noqa: E402
import coco_eval_ref as ref  # noqa: E402


def synthetic_epoch(images, k, classes, seed=0):
    """Ground truths: 1..13 per image (7 on average), sizes from small to large; detections: each object found with probability 0.7 as a
    jittered box with a high score, the remaining slots low-score clutter."""
    rng = np.random.default_rng(seed)
    gts, boxes, scores, labels = [], np.zeros((images, k, 4), np.float32), np.zeros((images, k), np.float32), np.zeros((images, k), np.int64)
    for n in range(images):
        g = int(rng.integers(1, 14))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (g, 2)))
        xy = rng.uniform(0, 512, (g, 2))
        gl = rng.integers(0, classes, g)
        gts.append((np.concatenate([xy, wh], 1), gl))
        found = np.flatnonzero(rng.random(g) < 0.7)[:k]
        m = len(found)
        jitter = 1 + rng.normal(0, 0.08, (m, 2))
        b = np.concatenate([xy[found] + rng.normal(0, 2, (m, 2)), wh[found] * jitter], 1)
        clutter = np.concatenate([rng.uniform(0, 512, (k - m, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (k - m, 2)))], 1)
        b = np.concatenate([b, clutter])
        boxes[n] = np.concatenate([b[:, :2], b[:, :2] + b[:, 2:]], 1)
        scores[n] = np.concatenate([rng.uniform(0.3, 1.0, m), rng.uniform(0.0, 0.4, k - m)])
        labels[n] = np.concatenate([gl[found], rng.integers(0, classes, k - m)])
    return boxes, scores, labels, gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ref-images", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    boxes, scores, labels, gts = synthetic_epoch(a.images, a.k, a.classes)
    d_boxes, d_scores, d_labels = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    targets = [{"boxes": b, "labels": l} for b, l in gts]

    def epoch(ev, n_images, timed):
        dev_ms, host_ms = [], []
        for i in range(0, n_images, a.batch):
            j = min(i + a.batch, n_images)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record()
            ev.update({"bboxes": d_boxes[i:j], "scores": d_scores[i:j], "labels": d_labels[i:j]}, targets[i:j])
            stop.record()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            if timed:
                stop.synchronize()
                dev_ms.append(start.elapsed_time(stop))
        return dev_ms, host_ms

    ev = cl.CocoEvaluator(a.classes)
    epoch(ev, min(a.images, 4 * a.batch), False)               # warm-up: library load, allocator, the kernels' first launch
    ev.get_metrics()
    ev.reset()
    dev_ms, host_ms = epoch(ev, a.images, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metrics = ev.get_metrics()
    metrics_ms = (time.perf_counter() - t0) * 1e3

    # the restatement on the host, over a subset; the evaluator over the same subset must agree bit for bit
    r = min(a.ref_images, a.images)
    t0 = time.perf_counter()
    want = ref.evaluate([(boxes[n], scores[n], labels[n]) for n in range(r)], gts[:r], a.classes)
    ref_s = time.perf_counter() - t0
    sub = cl.CocoEvaluator(a.classes)
    epoch(sub, r, False)
    got = sub.get_metrics()
    equal = np.array_equal(sub.precision, want["precision"]) and np.array_equal(sub.recall, want["recall"]) and got == want["metrics"]

    lines = [
        f"coco_eval_bench: {a.images} images, k = {a.k}, {a.classes} classes, {sum(len(l) for _, l in gts) / a.images:.2f} ground truths per image, batch {a.batch}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"update, per batch of {a.batch} (device time between events, list targets padded and uploaded per call): "
        f"median {np.median(dev_ms):.3f} ms, mean {np.mean(dev_ms):.3f} ms, max {np.max(dev_ms):.3f} ms over {len(dev_ms)} batches",
        f"update, host wall time of the call: median {np.median(host_ms):.3f} ms, sum over the epoch {np.sum(host_ms):.1f} ms",
        f"get_metrics (two sorts, one launch, one download, {ev._n} records): {metrics_ms:.2f} ms",
        f"whole epoch on the device path: {np.sum(host_ms) + metrics_ms:.1f} ms of host time",
        f"numpy restatement (tests/coco_eval_ref.py, plain Python) on the first {r} images: {ref_s:.2f} s "
        f"(linear in the images: about {ref_s * a.images / r:.0f} s for {a.images}); pycocotools is not available to time",
        f"evaluator == restatement on those {r} images, bit for bit: {equal}",
        "metrics of the synthetic epoch: " + ", ".join(f"{k} {v:.4f}" for k, v in metrics.items()),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not equal:
        sys.exit("the evaluator disagrees with the restatement")


if __name__ == "__main__":
    main()
