"""Times detection_loss (csrc/det_loss.hip) at the head shapes of the bench configurations, beside a torch-op restatement of the reference's
per-image / per-box loop (models/centernet.py:123-200) on the same device, and writes profiles/loss_bench.txt.

    python tools/loss_bench.py [--out profiles/loss_bench.txt]

Per call, device events, median of 20 after 5 warm-ups.  The first 4 images of every shape are checked against tests/loss_ref.py at the tolerance
of tests/test_gpu_loss.py (rtol 1e-8) before anything is timed; the torch loop (fp32, as the reference) is checked against it at 1e-4."""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import centernet_lightning_amd as cl  # noqa: E402
import loss_ref  # noqa: E402

SHAPES = {"C1 head (32 x 80 x 128 x 128, 20 boxes per image)": ((32, 80, 128, 128), 20),
          "C4 head (32 x 2 x 152 x 272, 40 boxes per image)": ((32, 2, 152, 272), 40)}
STRIDE = 4


def make(shape, per_image, seed=0):
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    heat = torch.from_numpy(rng.normal(-2.0, 2.0, shape).astype(np.float32)).cuda().contiguous(memory_format=torch.channels_last)
    box = torch.from_numpy(rng.uniform(0.0, 8.0, (N, 4, H, W)).astype(np.float32)).cuda().contiguous(memory_format=torch.channels_last)
    targets = []
    for _ in range(N):
        wh = rng.uniform(8.0, 160.0, (per_image, 2))
        c = np.stack([rng.uniform(0, W * STRIDE - 1, per_image), rng.uniform(0, H * STRIDE - 1, per_image)], 1)
        targets.append({"boxes": np.concatenate([c - wh / 2, wh], 1), "labels": rng.integers(0, C, per_image)})
    return heat, box, targets


def torch_loop(heat, box, targets):
    """The reference's loop with torch ops on the device: Gaussian windows box by box into a second N x C x H x W tensor, the focal loss as
    elementwise passes, the 3x3 samples gathered per image (cornernet radius, CornerNetFocalLoss, GIoULoss, weights 1)."""
    N, C, H, W = heat.shape
    dev = heat.device
    tmap = torch.zeros_like(heat)
    box_sum, n_dets, n_boxes = torch.zeros((), device=dev), 0, 0
    for n, t in enumerate(targets):
        b = np.asarray(t["boxes"], np.float64) / STRIDE
        if len(b) == 0:
            continue
        centres = np.rint(b[:, :2] + b[:, 2:] / 2).astype(int)
        idx, tgt = [], []
        for (x, y, w, h), (cx, cy), label, raw in zip(b, centres, t["labels"], np.asarray(t["boxes"], np.float64)):
            r = max(0, round(loss_ref.cornernet_radius(w, h, 0.3)))
            s = r / 3 + 1 / 6
            gy = torch.arange(-r, r + 1, device=dev).view(-1, 1)
            gx = torch.arange(-r, r + 1, device=dev).view(1, -1)
            g = torch.exp(-(gx.square() / (2 * s * s) + gy.square() / (2 * s * s)))
            g[g < torch.finfo(g.dtype).eps * g.max()] = 0
            le, to, ri, bo = min(cx, r), min(cy, r), min(W - cx, r + 1), min(H - cy, r + 1)
            win = tmap[n, int(label), cy - to:cy + bo, cx - le:cx + ri]
            torch.maximum(win, g[r - to:r + bo, r - le:r + ri], out=win)
            for sx in (cx - 1, cx, cx + 1):
                for sy in (cy - 1, cy, cy + 1):
                    if 0 <= sx <= W - 1 and 0 <= sy <= H - 1:
                        idx.append(sy * W + sx)
                        tgt.append([raw[0], raw[1], raw[0] + raw[2], raw[1] + raw[3]])
        n_dets += len(b)
        n_boxes += len(idx)
        i = torch.tensor(idx, device=dev)
        off = box[n].flatten(1).clamp_min(0)[:, i]
        px, py = (i % W) + 0.5, torch.div(i, W, rounding_mode="floor") + 0.5
        p = torch.stack([px - off[0], py - off[1], px + off[2], py + off[3]], -1) * STRIDE
        q = torch.tensor(tgt, device=dev, dtype=torch.float32)
        iw = (torch.minimum(p[:, 2], q[:, 2]) - torch.maximum(p[:, 0], q[:, 0])).clamp_min(0)
        ih = (torch.minimum(p[:, 3], q[:, 3]) - torch.maximum(p[:, 1], q[:, 1])).clamp_min(0)
        inter = iw * ih
        union = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1]) - inter
        enc = (torch.maximum(p[:, 2], q[:, 2]) - torch.minimum(p[:, 0], q[:, 0])) * (torch.maximum(p[:, 3], q[:, 3]) - torch.minimum(p[:, 1], q[:, 1]))
        box_sum = box_sum + (1 - (inter / (union + 1e-8) - (1 - union / enc))).sum()
    prob = torch.sigmoid(heat)
    pos = -torch.pow(1 - prob, 2) * torch.nn.functional.logsigmoid(heat) * tmap.eq(1).float()
    neg = -torch.pow(prob, 2) * torch.nn.functional.logsigmoid(-heat) * torch.pow(1 - tmap, 4)
    hm = (pos + neg).sum() / max(1, n_dets)
    bx = box_sum / max(1, n_boxes)
    return hm, bx, hm + bx


def timed(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.txt"))
    args = ap.parse_args()
    lines = [f"tools/loss_bench.py on {torch.cuda.get_device_name(0)}: per call, device events, median (min) of 20 after 5 warm-ups",
             "detection_loss: cornernet targets, cornernet_focal, giou, channels-last fp32 logits; padded device targets (no upload in the timed call)",
             "torch loop: the reference's per-image / per-box loop restated with torch ops on the same device (fp32), list-of-dicts targets", ""]
    for title, (shape, per_image) in SHAPES.items():
        heat, box, targets = make(shape, per_image)
        N = shape[0]
        G = per_image
        dev_t = (torch.from_numpy(np.stack([t["boxes"] for t in targets])).cuda(), torch.from_numpy(np.stack([t["labels"] for t in targets]).astype(np.int64)).cuda(),
                 torch.full((N,), G, dtype=torch.int32).cuda())
        # the first 4 images against the restatement
        got = cl.detection_loss(heat[:4], box[:4], targets[:4], stride=STRIDE)
        want = loss_ref.detection_loss(heat[:4].cpu().numpy(), box[:4].cpu().numpy(), [(t["boxes"], t["labels"]) for t in targets[:4]], stride=STRIDE)
        np.testing.assert_allclose(got["per_image"].cpu().numpy(), want["per_image"], rtol=1e-8, atol=0)
        np.testing.assert_allclose([float(got[k]) for k in ("heatmap", "box_2d", "total")], [want[k] for k in ("heatmap", "box_2d", "total")], rtol=1e-8, atol=0)
        loop = torch_loop(heat[:4], box[:4], targets[:4])
        np.testing.assert_allclose([float(v) for v in loop], [want[k] for k in ("heatmap", "box_2d", "total")], rtol=1e-4, atol=0)
        ours = timed(lambda: cl.detection_loss(heat, box, dev_t, stride=STRIDE))
        ours_list = timed(lambda: cl.detection_loss(heat, box, targets, stride=STRIDE))
        ref = timed(lambda: torch_loop(heat, box, targets), warmup=2, reps=5)
        elements = math.prod(shape)
        lines += [title, f"  first 4 images equal the numpy restatement at rtol 1e-8 (rows and totals); the torch loop at 1e-4",
                  f"  detection_loss, device targets      {ours[0]:9.3f} ms ({ours[1]:.3f})   {elements / ours[0] / 1e6:8.1f} G elements/s",
                  f"  detection_loss, list of dicts       {ours_list[0]:9.3f} ms ({ours_list[1]:.3f})   (host check, padding and one upload included)",
                  f"  torch loop (median of 5 after 2)    {ref[0]:9.3f} ms ({ref[1]:.3f})   x {ref[0] / ours[0]:.0f}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
