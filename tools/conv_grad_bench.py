"""Times the conv-gradient kernels (csrc/conv_grad.hip) at the head shapes of C1 (ResNet34 + simple neck, 32 x 512x512: maps 128 x 128) and of
C4 (ResNet34 + FPN tracking, 32 x 608x1088: maps 152 x 272) against torch's own autograd on the device for the same convs in fp32.

    python tools/conv_grad_bench.py [--out profiles/conv_grad_bench.txt] [--reps 20] [--only c1|c4]

wgrad   cnl_conv_wgrad_nhwc_f32 alone (both launches) against torch.nn.grad.conv2d_weight on channels-last tensors; the achieved rate counts the
        2 N H W Cout KH KW Cin operations of the GEMM over the call's time, as a fraction of the 157 TFLOP/s fp32-matrix peak.
head    the whole backward of one head (conv2d_nhwc: 3x3 + ReLU blocks, then the 1x1 out_conv; every weight and bias requires grad, the neck map
        does not) against torch.autograd on F.conv2d / relu with the same tensors.
        (The chains' weight gradients agree to about 1e-3 only, where single launches agree to 1e-6: a ReLU unit whose pre-activation rounds to the
        other side of zero moves one pixel's whole term in or out of a sum of random signs; both fp32 chains sit that far from a float64 chain.)
Times are device events around one call, median of --reps after 3 warm-up calls; random data (zeros would flatter both)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))

import torch
import torch.nn.functional as F

from centernet_lightning_amd import _lib, conv_grad

PEAK_TFLOPS = 157.0
SHAPES = {
    "c1": dict(N=32, H=128, W=128, convs=[(64, 256, 3), (256, 256, 3), (256, 80, 1)], head=[(64, 256, 3), (256, 256, 3), (256, 256, 3), (256, 80, 1)]),
    "c4": dict(N=32, H=152, W=272, convs=[(64, 256, 3), (256, 2, 1), (256, 4, 1), (256, 64, 1)], head=[(64, 256, 3), (256, 64, 1)]),
}


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def cl_tensor(N, C, H, W, gen):
    return torch.randn((N, H, W, C), device="cuda", generator=gen).permute(0, 3, 1, 2)


def bench_wgrad(N, H, W, cin, cout, k, reps, gen):
    x, dy = cl_tensor(N, cin, H, W, gen), cl_tensor(N, cout, H, W, gen)
    dz, _ = conv_grad.relu_grad(dy, None, want_bias=False)
    ours = lambda: conv_grad.conv_wgrad(x, cin, dz, dz.shape[3], cout, k, k)
    theirs = lambda: torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dy, padding=k // 2)
    a = ours().permute(0, 3, 1, 2)
    b = theirs()
    agree = float((a - b).abs().max() / b.abs().max())
    t_ours, t_min = timed(ours, reps)
    t_torch, _ = timed(theirs, reps)
    flops = 2.0 * N * H * W * cout * k * k * cin
    lib = _lib.load()
    return dict(shape=f"{N} x {H} x {W}, {cin} -> {cout}, {k}x{k}", slices=lib.cnl_conv_wgrad_slices(N, H, W, cin, cout, k, k), ms=t_ours, ms_min=t_min,
                tflops=flops / t_ours * 1e-9, torch_ms=t_torch, agree=agree)


def bench_head(N, H, W, layers, reps, gen):
    f = cl_tensor(N, layers[0][0], H, W, gen).contiguous(memory_format=torch.channels_last)
    ws = [(torch.randn((co, k, k, ci), device="cuda", generator=gen) * (2.0 / (k * k * ci)) ** 0.5).requires_grad_() for ci, co, k in layers]
    bs = [torch.zeros((co,), device="cuda").requires_grad_() for _, co, _ in layers]
    t = f
    for i, (w, b) in enumerate(zip(ws, bs)):
        t = conv_grad.conv2d_nhwc(t, w, b, relu=i < len(layers) - 1)
    g = torch.randn(t.shape, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    ours = lambda: torch.autograd.backward([t], [g], retain_graph=True)
    t_ours, _ = timed(ours, reps)
    got = [w.grad.clone() for w in ws]
    del t
    wt = [w.detach().permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_() for w in ws]
    bt = [b.detach().clone().requires_grad_() for b in bs]
    u = f
    for i, (w, b) in enumerate(zip(wt, bt)):
        u = F.conv2d(u, w, b, padding=w.shape[2] // 2)
        if i < len(layers) - 1:
            u = torch.relu(u)
    theirs = lambda: torch.autograd.backward([u], [g], retain_graph=True)
    t_torch, _ = timed(theirs, reps)
    # both accumulated 3 + reps backward passes into .grad: the same multiple of one gradient
    agree = max(float((a.permute(0, 3, 1, 2) - b.grad).abs().max() / b.grad.abs().max()) for a, b in zip(got, wt))
    return dict(shape=f"{N} x {H} x {W}, " + " / ".join(f"{ci}->{co} {k}x{k}" for ci, co, k in layers), ms=t_ours, torch_ms=t_torch, agree=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=sorted(SHAPES), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_grad_bench.py needs a HIP device: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"conv gradients on {torch.cuda.get_device_name(0)}: median of {args.reps} calls (device events), fp32, random data",
             f"wgrad = cnl_conv_wgrad_nhwc_f32 (both launches); fraction = achieved TFLOP/s over the {PEAK_TFLOPS:.0f} TFLOP/s fp32-matrix peak; "
             "torch = torch.nn.grad.conv2d_weight, channels-last; ratio = torch / ours (> 1: ours is faster)", ""]
    for name in ([args.only] if args.only else sorted(SHAPES)):
        s = SHAPES[name]
        for cin, cout, k in s["convs"]:
            r = bench_wgrad(s["N"], s["H"], s["W"], cin, cout, k, args.reps, gen)
            lines.append(f"{name} wgrad {r['shape']:36s} slices {r['slices']:4d}   {r['ms']:8.3f} ms (min {r['ms_min']:.3f})  {r['tflops']:6.1f} TFLOP/s = "
                         f"{r['tflops'] / PEAK_TFLOPS:5.1%} of peak   torch {r['torch_ms']:8.3f} ms   ratio {r['torch_ms'] / r['ms']:5.2f}   max rel diff {r['agree']:.1e}")
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
        r = bench_head(s["N"], s["H"], s["W"], s["head"], args.reps, gen)
        lines.append(f"{name} head backward {r['shape']}:   {r['ms']:8.3f} ms   torch {r['torch_ms']:8.3f} ms   ratio {r['torch_ms'] / r['ms']:5.2f}   "
                     f"max rel diff of the weight gradients {r['agree']:.1e}")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
