"""Letterbox micro-benchmark: N = 32 mixed-size uint8 frames -> one canvas batch.

  (a) the single launch: CenterNet.letterbox_uint8 (table upload + cnl_letterbox_bilinear_u8), and the kernel alone on a prebuilt table
  (b) the same canvas without it: canvas.fill + a Python loop of resize_uint8 per frame + a copy into the canvas

for 16 x 1920x1080 + 16 x 1280x720 frames -> 512 x 512, and the same frames -> 608 x 1088.  Device-event time per call over --reps calls,
--rounds rounds with (a) and (b) alternating; (b)'s spread over the rounds is the noise a difference has to exceed.  Three source sets
(> 256 MB together) rotate so that a call never finds its frames in the memory-side cache.  The kernel's must-move bytes (source rows
actually touched + canvas written) per second are printed beside the best "cold" rate of tools/hbm_read_peak on the same box
(hipcc --offload-arch=gfx950 -O3 tools/hbm_read_peak.hip -o tools/hbm_read_peak; skipped when the binary is absent).

    python tools/letterbox_bench.py [--reps 30] [--rounds 5] [--out profiles/letterbox_bench.txt]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
import centernet_lightning_amd as cl          # noqa: E402
from centernet_lightning_amd import _lib      # noqa: E402


def rows_touched(h, new_h):
    """Source rows the bilinear rule reads for new_h output rows (both taps, clipped to the image)."""
    scale = 1.0 / (new_h / h)
    sy = np.floor(((np.arange(new_h, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)
    return len(np.unique(np.concatenate([np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)])))


def must_move_bytes(geo, height, width, C=3):
    src = sum(rows_touched(h, nh) * w * C for (h, w, nh, nw, pt, pl) in geo)
    return src, len(geo) * height * width * C


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        fn(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stream_rate():
    exe = os.path.join(ROOT, "tools", "hbm_read_peak")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(m.group(1)) for ln in out.splitlines() if "cold" in ln for m in [re.search(r"([0-9.]+) TB/s", ln)] if m]
    return max(rates) if rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["command: python tools/letterbox_bench.py " + " ".join(sys.argv[1:]), "device: " + torch.cuda.get_device_name(0)]
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))      # host methods only
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    sets = [[torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device="cuda") for (h, w) in sizes] for _ in range(args.sets)]
    lines.append(f"frames: 16 x 1080x1920 + 16 x 720x1280 uint8 RGB, {args.sets} sets of {sum(f.numel() for f in sets[0]) / 1e6:.1f} MB rotating; "
                 f"{args.reps} calls per timing, {args.rounds} rounds, (a) and (b) alternating")
    peak = stream_rate()
    lines.append("tools/hbm_read_peak, best cold read-once stream on this box: " + (f"{peak:.3f} TB/s" if peak else "not measured (binary absent)"))
    ok = True
    for (height, width) in [(512, 512), (608, 1088)]:
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        prepared = [model.letterbox_uint8(s, height, width) for s in sets]
        geo = prepared[0][1].frames
        canvas = torch.empty_like(prepared[0][0])

        def a_full(r):
            model.letterbox_uint8(sets[r % len(sets)], height, width)

        def a_kernel(r):
            _lib.check(lib.cnl_letterbox_bilinear_u8(prepared[r % len(sets)][1].table.data_ptr(), canvas.data_ptr(), len(geo), height, width, 3, 0, stream))

        def b_loop(r):
            out = torch.empty((len(geo), height, width, 3), dtype=torch.uint8, device="cuda")
            out.fill_(0)
            for i, f in enumerate(sets[r % len(sets)]):
                h, w, nh, nw, pt, pl = geo[i]
                out[i, pt:pt + nh, pl:pl + nw] = model.resize_uint8(f[None], nh, nw)[0]
            return out

        assert torch.equal(b_loop(0), prepared[0][0]), "the loop and the single launch disagree"
        for fn in (a_full, a_kernel, b_loop):
            event_ms(fn, 10)
        ta, tk, tb = [], [], []
        for _ in range(args.rounds):
            ta.append(event_ms(a_full, args.reps))
            tb.append(event_ms(b_loop, args.reps))
            tk.append(event_ms(a_kernel, args.reps))
        src, dst = must_move_bytes(geo, height, width)
        med = lambda v: float(np.median(v))
        spread_b = max(tb) - min(tb)
        rate = (src + dst) / (med(tk) * 1e-3) / 1e12
        lines += [f"--- N = 32 -> {height} x {width}",
                  f"(a) letterbox_uint8 (upload + launch): median {med(ta) * 1e3:8.1f} us   rounds " + " ".join(f"{t * 1e3:.1f}" for t in ta),
                  f"(a) kernel alone                      : median {med(tk) * 1e3:8.1f} us   rounds " + " ".join(f"{t * 1e3:.1f}" for t in tk),
                  f"(b) fill + 32 x (resize_uint8 + copy) : median {med(tb) * 1e3:8.1f} us   rounds " + " ".join(f"{t * 1e3:.1f}" for t in tb)
                  + f"   spread {spread_b * 1e3:.1f} us",
                  f"(b) - (a) = {(med(tb) - med(ta)) * 1e3:.1f} us = {(med(tb) - med(ta)) / max(spread_b, 1e-9):.1f} x (b)'s spread; (b) / (a) = {med(tb) / med(ta):.1f} x",
                  f"must-move bytes: {src / 1e6:.1f} MB of source rows touched + {dst / 1e6:.1f} MB of canvas = {(src + dst) / 1e6:.1f} MB -> "
                  f"{rate:.3f} TB/s for the kernel alone" + (f" = {100 * rate / peak:.0f} % of the stream rate" if peak else "")]
        ok = ok and (med(tb) - med(ta)) > spread_b and max(ta) < min(tb)
    lines.append("condition ((a) faster than (b) by more than (b)'s spread, every round): " + ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
