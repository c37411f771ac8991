"""YUV letterbox micro-benchmark: N = 32 mixed 1080p / 720p frames -> one 512 x 512 RGB canvas batch, three ways.

  (a) letterbox_uint8 on the same frames already converted to packed RGB (the conversion itself is NOT timed: the path's lower bound)
  (b) letterbox_yuv420 on the NV12 surfaces (cnl_letterbox_yuv420_u8: the conversion inside the one launch)
  (c) what a user does without it: a torch-op NV12 -> RGB conversion of every frame on the device (the same integer rule: the result
      is asserted equal to (b)'s), then (a)

Device-event time per call, --reps calls per timing (>= 50), the median over --rounds rounds with (a), (b), (c) alternating, after a
warm-up; (c)'s spread over the rounds is the noise a difference has to exceed.  --sets source sets rotate so that a call does not find
its frames in the memory-side cache.  For (b) the kernel alone (prebuilt table) is timed too, and its must-move bytes (Y and chroma
rows actually touched + canvas written) per second are printed.

    python tools/yuv_bench.py [--reps 50] [--rounds 5] [--out profiles/yuv_letterbox_bench.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
import centernet_lightning_amd as cl          # noqa: E402
from centernet_lightning_amd import _lib      # noqa: E402


def source_rows(h, new_h):
    """Source rows the bilinear rule reads for new_h output rows (both taps, clipped to the frame)."""
    scale = 1.0 / (new_h / h)
    sy = np.floor(((np.arange(new_h, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)
    return np.unique(np.concatenate([np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)]))


def must_move_bytes(geo, height, width):
    """NV12: touched Y rows of w bytes + touched chroma rows of w bytes (w / 2 interleaved pairs), and the canvas."""
    src = 0
    for (h, w, nh, nw, pt, pl) in geo:
        rows = source_rows(h, nh)
        src += len(rows) * w + len(np.unique(rows >> 1)) * w
    return src, len(geo) * height * width * 3


def nv12_to_rgb_torch(frame, coef):
    """[h * 3 / 2, w] NV12 -> [h, w, 3] RGB with torch ops on the device: the integer rule of include/centernet_gfx950.h."""
    y_off, cy, cvr, cvg, cug, cub = coef
    h, w = frame.shape[0] // 3 * 2, frame.shape[1]
    yy = (frame[:h].to(torch.int32) - y_off).clamp_min_(0) * cy + (1 << 19)
    uv = frame[h:].view(h // 2, w // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
    u, v = uv[..., 0], uv[..., 1]
    rgb = torch.stack([(yy + cvr * v) >> 20, (yy + cvg * v + cug * u) >> 20, (yy + cub * u) >> 20], dim=-1)
    return rgb.clamp_(0, 255).to(torch.uint8)


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        fn(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    # (the arguments that bear on the figures; where the text goes is not one of them)
    lines = [f"command: python tools/yuv_bench.py --reps {args.reps} --rounds {args.rounds} --sets {args.sets}", "device: " + torch.cuda.get_device_name(0)]
    lib = _lib.load()
    coef = cl.yuv_coefficients("bt601", False)
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    height, width = 512, 512
    nv12 = [[torch.randint(0, 256, (h * 3 // 2, w), generator=g, dtype=torch.uint8, device="cuda") for (h, w) in sizes] for _ in range(args.sets)]
    rgb = [[nv12_to_rgb_torch(f, coef) for f in s] for s in nv12]
    lines.append(f"frames: 16 x 1080x1920 + 16 x 720x1280, {args.sets} sets rotating: NV12 {sum(f.numel() for f in nv12[0]) / 1e6:.1f} MB, "
                 f"packed RGB {sum(f.numel() for f in rgb[0]) / 1e6:.1f} MB per set; -> {height} x {width}; {args.reps} calls per timing, "
                 f"{args.rounds} rounds, (a) (b) (c) alternating")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    prepared = [cl.letterbox_yuv420(s, height, width) for s in nv12]
    geo = prepared[0][1].frames
    canvas = torch.empty_like(prepared[0][0])
    c_coef = (ctypes.c_int32 * 6)(*coef)

    def a_rgb(r):
        return cl.letterbox.letterbox_uint8(rgb[r % args.sets], height, width)[0]

    def b_yuv(r):
        return cl.letterbox_yuv420(nv12[r % args.sets], height, width)[0]

    def b_kernel(r):
        geom = prepared[r % args.sets][1]
        _lib.check(lib.cnl_letterbox_yuv420_u8(geom.yuv_table.data_ptr(), canvas.data_ptr(), len(geo), height, width, c_coef, 0, stream))

    def c_torch(r):
        return cl.letterbox.letterbox_uint8([nv12_to_rgb_torch(f, coef) for f in nv12[r % args.sets]], height, width)[0]

    assert torch.equal(a_rgb(0), b_yuv(0)) and torch.equal(c_torch(0), b_yuv(0)), "the three paths disagree"
    for fn in (a_rgb, b_yuv, b_kernel, c_torch):
        event_ms(fn, 10)
    ta, tb, tk, tc = [], [], [], []
    for _ in range(args.rounds):
        ta.append(event_ms(a_rgb, args.reps))
        tb.append(event_ms(b_yuv, args.reps))
        tc.append(event_ms(c_torch, args.reps))
        tk.append(event_ms(b_kernel, args.reps))
    src, dst = must_move_bytes(geo, height, width)
    med = lambda v: float(np.median(v))
    spread_c = max(tc) - min(tc)
    rate = (src + dst) / (med(tk) * 1e-3) / 1e12
    fmt = lambda v: " ".join(f"{t * 1e3:.1f}" for t in v)
    lines += [f"(a) letterbox_uint8 on ready RGB frames (upload + launch)   : median {med(ta) * 1e3:9.1f} us   rounds {fmt(ta)}",
              f"(b) letterbox_yuv420 on NV12 (upload + launch)              : median {med(tb) * 1e3:9.1f} us   rounds {fmt(tb)}",
              f"(b) kernel alone                                            : median {med(tk) * 1e3:9.1f} us   rounds {fmt(tk)}",
              f"(c) 32 x torch-op NV12 -> RGB, then letterbox_uint8         : median {med(tc) * 1e3:9.1f} us   rounds {fmt(tc)}   spread {spread_c * 1e3:.1f} us",
              f"(c) / (b) = {med(tc) / med(tb):.1f} x; (c) - (b) = {(med(tc) - med(tb)) * 1e3:.1f} us = {(med(tc) - med(tb)) / max(spread_c, 1e-9):.1f} x (c)'s spread",
              f"(b) / (a) = {med(tb) / med(ta):.2f} x (no bar: (b) reads half the bytes and does the conversion's integer work)",
              f"must-move bytes of (b): {src / 1e6:.1f} MB of Y and chroma rows touched + {dst / 1e6:.1f} MB of canvas = {(src + dst) / 1e6:.1f} MB -> "
              f"{rate:.3f} TB/s for the kernel alone"]
    ok = max(tb) < min(tc)
    lines.append("bar ((b) faster than (c), every round): " + ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
