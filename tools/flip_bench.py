"""Flip-test micro-benchmark: what the mirrored pass costs beyond its forward.

  (a) cnl_flip_merge_f32, all head maps in one launch, at the C1 shape (32 images: 2N = 64 maps of 80 + 4 channels, 128 x 128) and at
      the tracking shape (32 images: 2 + 4 + 64 channels, 152 x 272), on channels-last maps as the forward produces them;
  (b) the torch expression it replaces on the same tensors, per map: (a + b.flip(-1)[:, perm]) * 0.5 (no index for the maps whose
      channels stay).  Asserted bit-equal to (a) before anything is timed;
  (c) bytes moved per second by (a): two reads and one write per element, over its time, beside the read-once rate
      tools/hbm_read_peak.hip reports on the same box when its binary is given (--hbm-peak tools/hbm_read_peak; it runs first, as a
      child process);
  (d) one detection step, forward_uint8 + decode, on 32 frames of 512 x 512 (resnet34_simple): flip_test=True against the plain step,
      and against twice the plain step.

Device-event time per call, --reps calls per timing, the median and the spread over --rounds rounds with the variants alternating,
after a warm-up.  No bar: nothing gates on these figures.

    python tools/flip_bench.py [--reps 50] [--rounds 5] [--hbm-peak tools/hbm_read_peak] [--out profiles/flip_bench.txt]"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import centernet_lightning_amd as cl                       # noqa: E402
from yuv_bench import event_ms                             # noqa: E402

SHAPES = [("C1 detection", 32, 128, 128, (("heatmap", 80), ("box_2d", 4))),
          ("tracking", 32, 152, 272, (("heatmap", 2), ("box_2d", 4), ("reid", 64)))]


def hbm_read_peak(binary):
    """The best cold read-once rate (TB/s) the probe prints for its 512 MB buffers, or None."""
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300, check=True).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"^\s*cold\s+512 MB.*?([0-9.]+) TB/s\s*$", out, re.M)]
    return max(rates) if rates else None


def torch_merge(maps, N):
    out = {}
    for name, t in maps.items():
        a, b = t[:N], t[N:].flip(-1)
        if name == "box_2d":
            b = b[:, [2, 1, 0, 3]]
        out[name] = (a + b) * 0.5
    return out


def spread(v):
    return f"median {float(np.median(v)) * 1e3:9.1f} us   min {min(v) * 1e3:.1f}  max {max(v) * 1e3:.1f}   rounds " + " ".join(f"{x * 1e3:.1f}" for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hbm-peak", default=None, help="the binary built from tools/hbm_read_peak.hip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    peak = hbm_read_peak(args.hbm_peak) if args.hbm_peak else None      # before this process opens the device
    lines = [f"command: python tools/flip_bench.py --reps {args.reps} --rounds {args.rounds}" + (" --hbm-peak <binary of tools/hbm_read_peak.hip>" if args.hbm_peak else ""),
             "device: " + torch.cuda.get_device_name(0),
             f"{args.reps} calls per timing, {args.rounds} rounds, variants alternating; device events",
             "read-once HBM rate on this box (tools/hbm_read_peak.hip, best cold 512 MB line): " + (f"{peak:.3f} TB/s" if peak else "not measured")]
    med = lambda v: float(np.median(v))
    for title, N, H, W, heads in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        maps = {name: torch.randn((2 * N, H, W, C), device="cuda", generator=g).permute(0, 3, 1, 2) for name, C in heads}
        moved = sum(3 * 4 * N * C * H * W for _, C in heads)
        ours, theirs = cl.flip_merge(maps, N), torch_merge(maps, N)
        assert all(torch.equal(ours[k].view(torch.int32), theirs[k].view(torch.int32)) for k in maps), "the kernel and the torch expression disagree"
        del ours, theirs
        calls = [("(a) cnl_flip_merge_f32, one launch", lambda r: cl.flip_merge(maps, N)), ("(b) torch: (a + b.flip(-1)[:, perm]) * 0.5 per map", lambda r: torch_merge(maps, N))]
        for _, fn in calls:
            event_ms(fn, 5)
        t = [[] for _ in calls]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(calls):
                t[i].append(event_ms(fn, args.reps))
        lines.append(f"{title}: N = {N}, maps {H} x {W}, channels " + " + ".join(str(C) for _, C in heads) + f"; {moved / 1e6:.0f} MB moved per merge (2 reads + 1 write)")
        for (name, _), v in zip(calls, t):
            lines.append(f"  {name:<52} : {spread(v)}")
        rate = moved / (med(t[0]) * 1e-3) / 1e12
        lines.append(f"  (c) (a) moves {rate:.3f} TB/s" + (f" = {100.0 * rate / peak:.0f} % of the read-once rate" if peak else ""))
        lines.append(f"  (b) / (a): {med(t[1]) / med(t[0]):.2f} x" + ("" if med(t[1]) > med(t[0]) else "   (the kernel does NOT beat the torch expression)"))
        del maps
        torch.cuda.empty_cache()

    import bench
    torch.manual_seed(0)
    model = bench.synthetic_weights_(cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", bench.CONFIGS["simple"]))).cuda()
    frames = torch.randint(0, 256, (32, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))

    def step(flip):
        def run(r):
            return model.gather_detection2d(model.forward_uint8(frames, flip_test=True) if flip else model.forward_uint8(frames))
        return run
    calls = [("(d) forward_uint8 + decode, plain", step(False)), ("(d) forward_uint8 + decode, flip_test=True", step(True))]
    reps = max(args.reps // 5, 10)
    for _, fn in calls:
        event_ms(fn, 5)
    t = [[] for _ in calls]
    for _ in range(args.rounds):
        for i, (_, fn) in enumerate(calls):
            t[i].append(event_ms(fn, reps))
    lines.append(f"detection step, resnet34_simple, 32 frames of 512 x 512 uint8, {reps} steps per timing:")
    for (name, _), v in zip(calls, t):
        lines.append(f"  {name:<52} : median {med(v):8.3f} ms   rounds " + " ".join(f"{x:.3f}" for x in v))
    lines.append(f"  flip_test / plain: {med(t[1]) / med(t[0]):.3f} x; flip_test / (2 x plain): {med(t[1]) / (2 * med(t[0])):.3f} x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
