"""Crop micro-benchmark: 32 mixed 1080p / 720p frames x 100 boxes each -> 3200 crops of 128 x 64, from packed RGB and from NV12.

  (a) crop_detections: the one call (one pinned upload of 32 records, the record kernel, the gather)
  (b) what a user does without it: boxes to the host (a sync), a slice of the frame per box, letterbox_uint8 over the 3200 slices
      (one contiguous copy per slice, then one launch); for NV12 preceded by the torch-op NV12 -> RGB conversion of every frame
      (tools/yuv_bench.py's).  With keep_aspect=True (a) is asserted equal to (b).
  (c) cnl_crop_boxes_u8 alone (prebuilt frame records: both launches, no upload) for every rows-per-workgroup candidate: the product
      library and the variant libraries `make -C centernet-lightning_amd/csrc croprows ROWS=<r>` leaves under tools/ablibs/
      (those that exist are timed).

Device-event time per call, --reps calls per timing (>= 50), the median over --rounds rounds with the variants alternating, after a
warm-up; the (c) candidates are timed in rounds of their own behind 4 x --reps untimed calls, so that none of them follows (b)'s idle
device.  No bar: nothing gates on these figures.

    python tools/crop_bench.py [--reps 50] [--rounds 5] [--out profiles/crop_bench.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import centernet_lightning_amd as cl                       # noqa: E402
from centernet_lightning_amd import _gather, _lib          # noqa: E402
from yuv_bench import event_ms, nv12_to_rgb_torch          # noqa: E402

SIZE = (128, 64)
ROWS = (8, 16, 32, 64)


def person_boxes(sizes, k, seed):
    """k upright boxes per frame, 30..200 wide and 2..3 times as high, inside the frame: every slot is live."""
    rng = np.random.default_rng(seed)
    out = np.empty((len(sizes), k, 4), dtype=np.float32)
    for n, (h, w) in enumerate(sizes):
        bw = rng.uniform(30, 200, k)
        bh = np.minimum(bw * rng.uniform(2, 3, k), h - 1)
        x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        out[n] = np.stack([x1, y1, x1 + bw, y1 + bh], axis=-1)
    return out


def sliced_baseline(frames, boxes):
    """The parent's API: the boxes on the host, one slice per box, one letterbox_uint8 over the slices."""
    b = boxes.cpu().numpy()
    slices = []
    for n, f in enumerate(frames):
        for (x1, y1, x2, y2) in b[n]:
            slices.append(f[int(np.floor(y1)):int(np.ceil(y2)), int(np.floor(x1)):int(np.ceil(x2))])
    return cl.letterbox.letterbox_uint8(slices, SIZE[0], SIZE[1])[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    lines = [f"command: python tools/crop_bench.py --reps {args.reps} --rounds {args.rounds}", "device: " + torch.cuda.get_device_name(0)]
    coef = cl.yuv_coefficients("bt601", False)
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    N, k = len(sizes), 100
    nv12 = [torch.randint(0, 256, (h * 3 // 2, w), generator=g, dtype=torch.uint8, device="cuda") for (h, w) in sizes]
    rgb = [nv12_to_rgb_torch(f, coef) for f in nv12]
    boxes = torch.from_numpy(person_boxes(sizes, k, seed=1)).cuda()
    lines.append(f"workload: 16 x 1080x1920 + 16 x 720x1280 frames, {k} boxes each (30..200 wide, 2..3 times as high) -> {N * k} crops of "
                 f"{SIZE[0]} x {SIZE[1]}; {args.reps} calls per timing, {args.rounds} rounds, variants alternating")

    def a_rgb(r):
        return cl.crop_detections(rgb, boxes, SIZE, keep_aspect=True)[0]

    def a_nv12(r):
        return cl.crop_detections(nv12, boxes, SIZE, keep_aspect=True, pixel_format="nv12")[0]

    def b_rgb(r):
        return sliced_baseline(rgb, boxes)

    def b_nv12(r):
        return sliced_baseline([nv12_to_rgb_torch(f, coef) for f in nv12], boxes)

    want = b_rgb(0)
    assert torch.equal(a_rgb(0).flatten(0, 1), want) and torch.equal(a_nv12(0).flatten(0, 1), want) and torch.equal(b_nv12(0), want), \
        "the paths disagree"

    # (c): the C entry alone, per library
    windows = [(n, 0, 0, h, w, 1, 1, 0, 0) for n, (h, w) in enumerate(sizes)]
    rec_rgb, rec_yuv = np.zeros((N, 5), dtype=np.int64), np.zeros((N, 9), dtype=np.int64)
    _gather.pack_plain(rec_rgb, windows, [(f.data_ptr(), f.shape[1] * 3) for f in rgb])
    _gather.pack_yuv(rec_yuv, windows, [(f.data_ptr(), f.data_ptr() + h * w, f.data_ptr() + h * w + 1, w, w, 2) for f, (h, w) in zip(nv12, sizes)])
    t_rgb, t_yuv = torch.from_numpy(rec_rgb).cuda(), torch.from_numpy(rec_yuv).cuda()
    out = torch.empty((N, k) + SIZE + (3,), dtype=torch.uint8, device="cuda")
    win = torch.empty((N, k, 4), dtype=torch.int32, device="cuda")
    records = torch.empty((N * k * 9,), dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    c_coef = (ctypes.c_int32 * 6)(*coef)
    libs = [("product library", _lib.load())]
    for r in ROWS:
        path = os.path.join(ROOT, "tools", "ablibs", f"libcnl_croprows{r}.so")
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            lib.cnl_crop_boxes_u8.restype, lib.cnl_crop_boxes_u8.argtypes = _lib._SIGNATURES["cnl_crop_boxes_u8"]
            libs.append((f"{r:2d} rows per workgroup", lib))

    def entry(lib, yuv):
        def run(r):
            rc = lib.cnl_crop_boxes_u8((t_yuv if yuv else t_rgb).data_ptr(), boxes.data_ptr(), None, 0.0, None, N, k, 3, c_coef if yuv else None, 0.0, 1,
                                       records.data_ptr(), win.data_ptr(), out.data_ptr(), SIZE[0], SIZE[1], 0, stream)
            assert rc == 0, rc
        return run

    kernels = []
    for name, lib in libs:
        for yuv in (False, True):
            fn = entry(lib, yuv)
            fn(0)
            assert torch.equal(out.flatten(0, 1), want), f"{name}: wrong crops"
            kernels.append((f"(c) cnl_crop_boxes_u8 alone, {'NV12' if yuv else 'RGB '}, {name}", fn))
    calls = [("(a) crop_detections, packed RGB (upload + 2 launches)", a_rgb), ("(a) crop_detections, NV12 (upload + 2 launches)", a_nv12),
             ("(b) boxes to host, 3200 slices, letterbox_uint8, packed RGB", b_rgb),
             ("(b) 32 x torch-op NV12 -> RGB, then the same", b_nv12)]
    timed = calls + kernels
    for _, fn in timed:
        event_ms(fn, 5)
    t = [[] for _ in timed]
    # the launch-shape candidates in rounds of their own, the device kept busy in front of each round: (b) leaves it idle most of the
    # time, and timed right behind (b) the product library came out 15 % behind the 32-row variant, which is the same code
    for _ in range(args.rounds):
        event_ms(kernels[0][1], 4 * args.reps)
        for i, (_, fn) in enumerate(kernels):
            t[len(calls) + i].append(event_ms(fn, args.reps))
    for _ in range(args.rounds):
        for i, (_, fn) in enumerate(calls):
            t[i].append(event_ms(fn, args.reps))
    med = lambda v: float(np.median(v))
    width = max(len(name) for name, _ in timed)
    for (name, _), v in zip(timed, t):
        lines.append(f"{name:<{width}} : median {med(v) * 1e3:10.1f} us   rounds " + " ".join(f"{x * 1e3:.1f}" for x in v))
    lines.append(f"(b) / (a): packed RGB {med(t[2]) / med(t[0]):.1f} x, NV12 {med(t[3]) / med(t[1]):.1f} x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
