"""Times the re-ID loss (csrc/reid_loss.hip: cnl_reid_loss_f64 / cnl_reid_loss_grad_f32) at the head shape of the tracking bench configuration C4
(32 x 64 x 152 x 272, Gmax = 128 boxes per image, every slot a live row): forward, and forward + backward, through ReIDLoss, beside a torch-op
restatement of the reference on the device (gather, the nn.Sequential in fp32 — two rocBLAS GEMMs —, CrossEntropyLoss, autograd), and writes
profiles/reid_loss_bench.txt.

    python tools/reid_loss_bench.py [--out profiles/reid_loss_bench.txt]

K = 800 (configs/tracking_resnet34_fpn.yaml) and 14455 (the identity count of FairMOT's training mix).  Per call, device events, median of 20 after 5
warm-ups.  Before anything is timed the value and the map's gradient of both paths are compared (the torch path is fp32: 1e-3 of the largest entry).
The two paths do not compute the same thing at the same precision: the HIP path is float64 with fixed summation orders (the same bits on every run)
and never writes the logits; the torch path is fp32, writes the R x K logits, and its scatter backward adds with atomics."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import centernet_lightning_amd as cl  # noqa: E402
import loss_bench  # noqa: E402

STRIDE = 4
SHAPE, GMAX = (32, 64, 152, 272), 128
IDS = (800, 14455)


def make(K, seed=0):
    N, D, H, W = SHAPE
    rng = np.random.default_rng(seed)
    reid = torch.from_numpy(rng.normal(0, 1, SHAPE).astype(np.float32)).cuda().contiguous(memory_format=torch.channels_last)
    centres = np.stack([rng.uniform(0, W, (N, GMAX)), rng.uniform(0, H, (N, GMAX))], -1) * STRIDE
    sizes = rng.uniform(8, 120, (N, GMAX, 2))
    boxes = np.concatenate([centres - sizes / 2, sizes], -1)
    ids = rng.integers(0, K, (N, GMAX)).astype(np.int64)
    targets = {"boxes": torch.from_numpy(boxes).cuda(), "ids": torch.from_numpy(ids).cuda(), "count": torch.full((N,), GMAX, dtype=torch.int32).cuda()}
    return reid, targets


def torch_path(module, reid, targets):
    """The reference's compute_loss with torch ops: trunc cells, gather, the Sequential, cross entropy with reduction none, mask all ones."""
    N, D, H, W = reid.shape
    b = targets["boxes"]
    x = ((b[..., 0] + b[..., 2] / 2) / STRIDE).long()
    y = ((b[..., 1] + b[..., 3] / 2) / STRIDE).long()
    index = (y * W + x).unsqueeze(1).expand(N, D, -1)
    rows = torch.gather(reid.reshape(N, D, -1), -1, index).swapaxes(1, 2).reshape(-1, D)
    logits = module.classifier(rows)
    loss = torch.nn.functional.cross_entropy(logits, targets["ids"].reshape(-1), reduction="none")
    return loss.sum() / (loss.numel() + 1e-8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reid_loss_bench.txt"))
    args = ap.parse_args()
    N, D, H, W = SHAPE
    lines = [f"tools/reid_loss_bench.py on {torch.cuda.get_device_name(0)}: per call, device events, median (min) of 20 after 5 warm-ups",
             f"C4 head: reid {N} x {D} x {H} x {W} channels-last fp32, Gmax = {GMAX}, every slot a live row ({N * GMAX} rows), training mode, device targets",
             "HIP: ReIDLoss (float64 on the fp32 values, fixed orders, logits never stored); torch: gather + nn.Sequential (fp32) + cross_entropy + autograd", ""]
    for K in IDS:
        torch.manual_seed(0)
        module = cl.ReIDLoss(D, K, stride=STRIDE).cuda()
        twin = cl.ReIDLoss(D, K, stride=STRIDE).cuda()
        twin.load_state_dict(module.state_dict())
        reid, targets = make(K)
        x = reid.clone().requires_grad_()
        params = [x] + list(module.parameters())

        def step(fn, leaves):
            for p in leaves:
                p.grad = None
            fn().backward()

        ours = module({"reid": x}, targets)["reid"]
        ours.backward()
        g_ours = x.grad.clone()
        x.grad = None
        theirs = torch_path(twin, x, targets)
        theirs.backward()
        assert abs(float(ours.detach()) - float(theirs.detach())) <= 1e-3 * abs(float(ours.detach())), (float(ours.detach()), float(theirs.detach()))
        assert float((g_ours - x.grad).abs().max()) <= 1e-3 * float(g_ours.abs().max())
        with torch.no_grad():
            fwd = loss_bench.timed(lambda: module({"reid": reid}, targets))
            fwd_t = loss_bench.timed(lambda: torch_path(twin, reid, targets))
        both = loss_bench.timed(lambda: step(lambda: module({"reid": x}, targets)["reid"], params))
        both_t = loss_bench.timed(lambda: step(lambda: torch_path(twin, x, targets), [x] + list(twin.parameters())))
        lines += [f"K = {K}   (value {float(ours.detach()):.6f}; torch fp32 {float(theirs.detach()):.6f})",
                  f"  ReIDLoss forward                     {fwd[0]:9.3f} ms ({fwd[1]:.3f})",
                  f"  torch ops forward                    {fwd_t[0]:9.3f} ms ({fwd_t[1]:.3f})   HIP / torch = {fwd[0] / fwd_t[0]:.2f}",
                  f"  ReIDLoss forward + backward          {both[0]:9.3f} ms ({both[1]:.3f})",
                  f"  torch ops forward + backward         {both_t[0]:9.3f} ms ({both_t[1]:.3f})   HIP / torch = {both[0] / both_t[0]:.2f}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
