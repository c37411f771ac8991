"""Overlay micro-benchmark: 32 mixed 1080p / 720p frames x 100 boxes each, drawn in place (thickness 2, number tags at scale 2) onto
packed RGB frames and onto NV12 surfaces.

  (a) draw_detections(..., inplace=True): the one call (one pinned upload of 32 records and the palette, the record kernel, the paint
      kernel)
  (b) what a user does without it: boxes to the host (a sync), then per box four torch slice assignments (the sides of the ring) on the
      device frame.  Packed RGB only: torch has no equivalent for an NV12 surface (the chroma planes would need the chroma rule), and
      (b) draws no tags, so it does LESS than (a).  Its ring is asserted equal to (a)'s without tags.
  (c) cnl_draw_boxes_u8 alone (prebuilt frame records and palette: both launches, no upload), packed RGB and NV12, and the bytes it
      touches per second: the bytes of a black frame that the call makes non-zero (every palette byte is non-zero), over its time.

Device-event time per call, --reps calls per timing (>= 50; (b) takes a tenth as many: it is three orders slower), the median over
--rounds rounds with the variants alternating, after a warm-up.  No bar: nothing gates on these figures.

    python tools/overlay_bench.py [--reps 50] [--rounds 5] [--out profiles/overlay_bench.txt]"""
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
from crop_bench import person_boxes                        # noqa: E402
from yuv_bench import event_ms                             # noqa: E402

THICKNESS, TAG_SCALE = 2, 2
PALETTE = [tuple(max(v, 1) for v in c) for c in cl.DEFAULT_PALETTE]       # no zero byte: a painted byte of a black frame is non-zero


def sliced_baseline(frames, boxes, labels, palette):
    """Boxes and labels to the host, then the ring of every box as four slice assignments (t = 2: the ring grows two pixels inwards)."""
    b, l = boxes.cpu().numpy(), labels.cpu().numpy()
    for n, f in enumerate(frames):
        H, W = f.shape[:2]
        for j in range(b.shape[1] - 1, -1, -1):
            x1, y1, x2, y2 = (int(v) for v in np.rint(b[n, j]))
            c = palette[l[n, j] % len(palette)]
            xa, xb, ya, yb = max(x1, 0), min(x2, W - 1) + 1, max(y1, 0), min(y2, H - 1) + 1
            f[max(y1, 0):min(y1 + 2, yb), xa:xb] = c
            f[max(y2 - 1, ya):yb, xa:xb] = c
            f[ya:yb, max(x1, 0):min(x1 + 2, xb)] = c
            f[ya:yb, max(x2 - 1, xa):xb] = c
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    lines = [f"command: python tools/overlay_bench.py --reps {args.reps} --rounds {args.rounds}", "device: " + torch.cuda.get_device_name(0)]
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    N, k = len(sizes), 100
    rgb = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for (h, w) in sizes]
    nv12 = [torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for (h, w) in sizes]
    boxes = torch.from_numpy(person_boxes(sizes, k, seed=1)).cuda()
    rng = np.random.default_rng(2)
    labels = torch.from_numpy(rng.integers(0, 80, (N, k))).cuda()
    numbers = torch.from_numpy(rng.integers(0, 1000, (N, k)).astype(np.int32)).cuda()
    pal_t = torch.tensor(PALETTE, dtype=torch.uint8, device="cuda")
    lines.append(f"workload: 16 x 1080x1920 + 16 x 720x1280 frames, {k} boxes each (30..200 wide, 2..3 times as high), thickness {THICKNESS}, "
                 f"tags of 1..3 digits at scale {TAG_SCALE}; {args.reps} calls per timing, {args.rounds} rounds, variants alternating")

    def a_rgb(r):
        return cl.draw_detections(rgb, boxes, labels=labels, numbers=numbers, palette=PALETTE, thickness=THICKNESS, tag_scale=TAG_SCALE, inplace=True)

    def a_nv12(r):
        return cl.draw_detections(nv12, boxes, labels=labels, numbers=numbers, palette=PALETTE, thickness=THICKNESS, tag_scale=TAG_SCALE,
                                  pixel_format="nv12", inplace=True)

    def b_rgb(r):
        return sliced_baseline(rgb, boxes, labels, pal_t)

    # (b)'s rings are (a)'s without tags
    want = [f.clone() for f in cl.draw_detections(rgb, boxes, labels=labels, palette=PALETTE, thickness=THICKNESS, tag_scale=0)]
    b_rgb(0)
    assert all(torch.equal(x, y) for x, y in zip(rgb, want)), "the baseline draws other rings"
    for f in rgb:
        f.zero_()

    # (c): the C entry alone
    windows = [(n, 0, 0, h, w, 1, 1, 0, 0) for n, (h, w) in enumerate(sizes)]
    rec_rgb, rec_yuv = np.zeros((N, 5), dtype=np.int64), np.zeros((N, 9), dtype=np.int64)
    _gather.pack_plain(rec_rgb, windows, [(f.data_ptr(), f.shape[1] * 3) for f in rgb])
    _gather.pack_yuv(rec_yuv, windows, [(f.data_ptr(), f.data_ptr() + h * w, f.data_ptr() + h * w + 1, w, w, 2) for f, (h, w) in zip(nv12, sizes)])
    t_rgb, t_yuv = torch.from_numpy(rec_rgb).cuda(), torch.from_numpy(rec_yuv).cuda()

    def palette_words(colours, text):
        a = np.zeros((len(colours) + 1, 4), dtype=np.uint8)
        a[:-1, :3] = colours
        a[-1, :3] = text
        return torch.from_numpy(a.view(np.uint32).reshape(-1).astype(np.int64)).to(torch.int32).cuda()
    p_rgb, p_yuv = palette_words(PALETTE, (255, 255, 255)), palette_words([cl.rgb_to_yuv(c) for c in PALETTE], cl.rgb_to_yuv((255, 255, 255)))
    records = torch.empty((N * k * 8,), dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()

    def entry(yuv):
        def run(r):
            rc = lib.cnl_draw_boxes_u8((t_yuv if yuv else t_rgb).data_ptr(), boxes.data_ptr(), labels.data_ptr(), numbers.data_ptr(), None, 0.0, None,
                                       N, k, 3, int(yuv), (p_yuv if yuv else p_rgb).data_ptr(), len(PALETTE), THICKNESS, 0, TAG_SCALE, 1080, 1920,
                                       records.data_ptr(), stream)
            assert rc == 0, rc
        return run
    touched = []
    for yuv, frames, fn in ((False, rgb, a_rgb), (True, nv12, a_nv12)):
        entry(yuv)(0)
        torch.cuda.synchronize()
        touched.append(sum(int((f != 0).sum()) for f in frames))
        alone = [f.clone() for f in frames]
        for f in frames:
            f.zero_()
        fn(0)
        assert all(torch.equal(x, y) for x, y in zip(frames, alone)), "the entry point and draw_detections disagree"
    total = [sum(f.numel() for f in rgb), sum(f.numel() for f in nv12)]
    lines.append(f"bytes touched per call: packed RGB {touched[0]} of {total[0]} ({100.0 * touched[0] / total[0]:.2f} %), "
                 f"NV12 {touched[1]} of {total[1]} ({100.0 * touched[1] / total[1]:.2f} %)")

    calls = [("(a) draw_detections in place, packed RGB (upload + 2 launches)", a_rgb, args.reps),
             ("(a) draw_detections in place, NV12 (upload + 2 launches)", a_nv12, args.reps),
             ("(b) boxes to host, 4 slice assignments per box, packed RGB, no tags", b_rgb, max(args.reps // 10, 5)),
             ("(c) cnl_draw_boxes_u8 alone, packed RGB", entry(False), args.reps), ("(c) cnl_draw_boxes_u8 alone, NV12", entry(True), args.reps)]
    for _, fn, _ in calls:
        event_ms(fn, 3)
    t = [[] for _ in calls]
    for _ in range(args.rounds):
        for i, (_, fn, reps) in enumerate(calls):
            t[i].append(event_ms(fn, reps))
    med = lambda v: float(np.median(v))
    width = max(len(name) for name, _, _ in calls)
    for (name, _, _), v in zip(calls, t):
        lines.append(f"{name:<{width}} : median {med(v) * 1e3:10.1f} us   rounds " + " ".join(f"{x * 1e3:.1f}" for x in v))
    lines.append(f"(b) / (a), packed RGB: {med(t[2]) / med(t[0]):.1f} x" + ("" if med(t[2]) > med(t[0]) else "   (the call does NOT beat the baseline)"))
    lines.append(f"(c) bytes touched per second: packed RGB {touched[0] / med(t[3]) * 1e3 / 1e9:.2f} GB/s, NV12 {touched[1] / med(t[4]) * 1e3 / 1e9:.2f} GB/s "
                 "(painted bytes only; the kernel also reads them, and every workgroup reads the 100 rectangles of its frame)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
