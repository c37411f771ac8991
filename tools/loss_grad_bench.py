"""Times the gradient of the detection loss (csrc/det_loss.hip: cnl_detection_loss_grad_f32) at the head shapes of the bench configurations:
the gradient call alone, forward + backward through DetectionLoss, and forward + backward of the torch-op restatement of the reference's
per-image / per-box loop that tools/loss_bench.py holds (imported from there), and writes profiles/loss_grad_bench.txt.

    python tools/loss_grad_bench.py [--out profiles/loss_grad_bench.txt]

Per call, device events, median of 20 after 5 warm-ups (the torch loop: 5 after 2).  Before anything is timed the gradients of the first 2 images are
checked against tests/loss_grad_ref.py at the bound of tests/test_gpu_loss_grad.py (one fp32 ulp + 1e-12 max|ref|), and the torch loop's own fp32
autograd gradients against them at 1e-3 of the largest entry.  The "share of HBM" is (logits read once + both gradients written once) / time over
the 6.3 TB/s a float4 copy reaches on an MI355X (8.0 TB/s on paper)."""
import argparse
import math
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
import loss_grad_ref  # noqa: E402

STRIDE = loss_bench.STRIDE
HBM_TBS = 6.3


def check(heat, box, targets, dev_t):
    """The first 2 images against the restatement (the test's bound); the torch loop's autograd against the restatement at 1e-3."""
    h, b = heat[:2].contiguous(memory_format=torch.channels_last), box[:2].contiguous(memory_format=torch.channels_last)
    got = cl.detection_loss_grad(h, b, tuple(t[:2] for t in dev_t), stride=STRIDE)
    want = loss_grad_ref.detection_loss_grad(h.cpu().numpy(), b.cpu().numpy(), [(t["boxes"], t["labels"]) for t in targets[:2]], stride=STRIDE)
    for key in ("heatmap_grad", "box_2d_grad"):
        ref64 = want[key + "64"]
        ref = ref64.astype(np.float32)
        tol = np.spacing(np.abs(ref)).astype(np.float64) + 1e-12 * np.abs(ref64).max()
        assert (np.abs(got[key].cpu().numpy().astype(np.float64) - ref) <= tol).all(), key
    hl, bl = h.clone().requires_grad_(), b.clone().requires_grad_()
    loss_bench.torch_loop(hl, bl, targets[:2])[2].backward()
    for g, key in ((hl.grad, "heatmap_grad"), (bl.grad, "box_2d_grad")):
        assert np.abs(g.cpu().numpy() - want[key]).max() <= 1e-3 * np.abs(want[key]).max(), key


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_grad_bench.txt"))
    args = ap.parse_args()
    lines = [f"tools/loss_grad_bench.py on {torch.cuda.get_device_name(0)}: per call, device events, median (min) of 20 after 5 warm-ups",
             "cornernet targets, cornernet_focal, giou, weights 1; channels-last fp32 logits and box values; padded device targets",
             "torch loop: tools/loss_bench.py's restatement of the reference's per-image / per-box loop with torch ops (fp32), its autograd backward", ""]
    for title, (shape, per_image) in loss_bench.SHAPES.items():
        heat, box, targets = loss_bench.make(shape, per_image)
        N = shape[0]
        dev_t = (torch.from_numpy(np.stack([t["boxes"] for t in targets])).cuda(), torch.from_numpy(np.stack([t["labels"] for t in targets]).astype(np.int64)).cuda(),
                 torch.full((N,), per_image, dtype=torch.int32).cuda())
        check(heat, box, targets, dev_t)
        criterion = cl.DetectionLoss(stride=STRIDE)
        hl, bl = heat.clone().requires_grad_(), box.clone().requires_grad_()

        def step(fn, tg):
            hl.grad = bl.grad = None
            fn(hl, bl, tg).backward()

        grad = loss_bench.timed(lambda: cl.detection_loss_grad(heat, box, dev_t, stride=STRIDE))
        heat_only = loss_bench.timed(lambda: cl.detection_loss_grad(heat, box, dev_t, stride=STRIDE, want=("heatmap",)))
        box_only = loss_bench.timed(lambda: cl.detection_loss_grad(heat, box, dev_t, stride=STRIDE, want=("box_2d",)))
        fwd = loss_bench.timed(lambda: cl.detection_loss(heat, box, dev_t, stride=STRIDE))
        both = loss_bench.timed(lambda: step(lambda h, b, t: criterion({"heatmap": h, "box_2d": b}, t)["total"], dev_t))
        both_list = loss_bench.timed(lambda: step(lambda h, b, t: criterion({"heatmap": h, "box_2d": b}, t)["total"], targets))
        loop = loss_bench.timed(lambda: step(lambda h, b, t: loss_bench.torch_loop(h, b, t)[2], targets), warmup=2, reps=5)
        moved = (2 * math.prod(shape) + N * 4 * shape[2] * shape[3]) * 4
        share = lambda ms: f"{moved / (ms * 1e-3) / 1e12:5.2f} TB/s = {100 * moved / (ms * 1e-3) / 1e12 / HBM_TBS:4.1f} % of {HBM_TBS} TB/s"
        lines += [title, "  first 2 images: both gradients equal the numpy restatement to one fp32 ulp; the torch loop's autograd to 1e-3 of the largest entry",
                  f"  detection_loss_grad, both gradients        {grad[0]:9.3f} ms ({grad[1]:.3f})   {moved / 1e6:6.1f} MB read once + written once: {share(grad[0])}",
                  f"    heatmap gradient only                    {heat_only[0]:9.3f} ms ({heat_only[1]:.3f})",
                  f"    box gradient only                        {box_only[0]:9.3f} ms ({box_only[1]:.3f})",
                  f"  detection_loss (the value, for scale)      {fwd[0]:9.3f} ms ({fwd[1]:.3f})",
                  f"  DetectionLoss forward + backward           {both[0]:9.3f} ms ({both[1]:.3f})   (device targets; autograd's bookkeeping included)",
                  f"  DetectionLoss forward + backward, lists    {both_list[0]:9.3f} ms ({both_list[1]:.3f})   (host check, padding and one upload included)",
                  f"  torch loop forward + backward (5 after 2)  {loop[0]:9.3f} ms ({loop[1]:.3f})   x {loop[0] / both[0]:.0f}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
