"""Augmentation micro-benchmark: 32 mixed 1080p / 720p RGB frames with 40 boxes each -> 32 augmented canvases of 512 x 512 and of
608 x 1088 and their targets, with and without mosaic (flip 0.5, ColorJitter 0.4 / 0.4 / 0.4, hue 0.1, Cutout 10 x 60 x 60).

  (a) augment_batch: the one call (one pinned upload: frame records + plan; cnl_augment_u8 + cnl_augment_boxes_f64), targets on the device
  (b) a torch-op restatement on the device, the same plan, per image: slice, F.interpolate (bilinear, so NOT the same bytes), flip, a
      matrix multiply, hole fills, and the box arithmetic of the rule with a boolean-mask compaction.  What a user writes without (a).
  (c) cnl_augment_u8 alone (prebuilt device records, no upload), with the bytes it must move: the canvas written once plus the source
      window rows it touches (at most two source rows per canvas row), against the time -> a rate to compare with the letterbox kernel's
      on the same shapes.

Per call: device events around ONE call, the median of --calls calls (>= 20), after a warm-up of every variant, the variants alternating.
No bar: nothing gates on these figures.

    python tools/augment_bench.py [--calls 20] [--out profiles/augment_bench.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
import centernet_lightning_amd as cl                       # noqa: E402
from centernet_lightning_amd import _frames, _gather, _lib, augment        # noqa: E402

SETTINGS = dict(flip=0.5, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, cutout=(10, 60, 60))
BOXES = 40


def call_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_targets(sizes, seed):
    rng = np.random.default_rng(seed)
    boxes = np.zeros((len(sizes), BOXES, 4))
    for n, (h, w) in enumerate(sizes):
        bw, bh = rng.uniform(20, 300, BOXES), rng.uniform(40, 500, BOXES)
        boxes[n] = np.stack([rng.uniform(0, w - bw), rng.uniform(0, h - bh), bw, bh], axis=-1)
    return {"boxes": torch.from_numpy(boxes).cuda(), "labels": torch.from_numpy(rng.integers(0, 80, (len(sizes), BOXES))).cuda(),
            "count": torch.full((len(sizes),), BOXES, dtype=torch.int32, device="cuda")}


def torch_baseline(frames, plan, targets, fill, hole_fill):
    """The same plan with torch ops, one image and one placement at a time (bilinear interpolation in fp32: close to, not equal to, the
    integer resize)."""
    N, H, W = len(plan), plan.height, plan.width
    canvas = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    canvas[...] = torch.tensor(fill, dtype=torch.uint8, device="cuda")
    Gout = plan.max_place * BOXES
    out_boxes = torch.zeros((N, Gout, 4), dtype=torch.float64, device="cuda")
    out_labels = torch.zeros((N, Gout), dtype=torch.int64, device="cuda")
    out_count = torch.zeros((N,), dtype=torch.int32, device="cuda")
    for n in range(N):
        kept_b, kept_l = [], []
        for p in range(int(plan.n_place[n])):
            f = int(plan.frame[n, p])
            x0, y0, w, h = (int(v) for v in plan.window[n, p])
            dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
            q = torch.from_numpy(plan.colour[n, p].astype(np.float32) / 4096.0).cuda()
            win = frames[f][y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].float()
            r = F.interpolate(win, size=(dh, dw), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
            if plan.flip[n, p]:
                r = r.flip(1)
            r = r @ q[:9].view(3, 3).T + q[9:]
            canvas[n, dy0:dy0 + dh, dx0:dx0 + dw] = r.round().clamp(0, 255).to(torch.uint8)
            b = targets["boxes"][f]
            sx, sy = dw / w, dh / h
            u1, u2 = (b[:, 0] - x0) * sx, (b[:, 0] + b[:, 2] - x0) * sx
            v1, v2 = (b[:, 1] - y0) * sy, (b[:, 1] + b[:, 3] - y0) * sy
            if plan.flip[n, p]:
                u1, u2 = dw - u2, dw - u1
            cu1, cu2, cv1, cv2 = u1.clamp(0, dw), u2.clamp(0, dw), v1.clamp(0, dh), v2.clamp(0, dh)
            cw, ch = cu2 - cu1, cv2 - cv1
            keep = (cw > 0) & (ch > 0) & (cw * ch >= 1.0) & (targets["labels"][f] >= 0)
            kept_b.append(torch.stack([dx0 + cu1, dy0 + cv1, cw, ch], dim=-1)[keep])
            kept_l.append(targets["labels"][f][keep])
        for (hx, hy, hw, hh) in plan.holes[n].tolist():
            if hw > 0 and hh > 0:
                canvas[n, max(hy, 0):max(min(hy + hh, H), 0), max(hx, 0):max(min(hx + hw, W), 0)] = torch.tensor(hole_fill, dtype=torch.uint8, device="cuda")
        kb, kl = torch.cat(kept_b), torch.cat(kept_l)
        out_boxes[n, :kb.shape[0]], out_labels[n, :kb.shape[0]], out_count[n] = kb, kl, kb.shape[0]      # (a boolean mask: one sync per placement)
    return canvas, {"boxes": out_boxes, "labels": out_labels, "count": out_count}


def must_move_bytes(plan):
    """Canvas bytes written once + source bytes touched: per placement the window's rows that the dh output rows tap (at most 2 dh of its h
    rows), whole window rows."""
    total = len(plan) * plan.height * plan.width * 3
    for n in range(len(plan)):
        for p in range(int(plan.n_place[n])):
            _, _, w, h = (int(v) for v in plan.window[n, p])
            total += min(h, 2 * int(plan.dest[n, p, 3])) * w * 3
    return total


def kernel_alone(frames, plan, fill, hole_fill):
    """-> (fn, canvas): cnl_augment_u8 on records uploaded once."""
    src = _frames.open_frames(frames, "rgb", "augment_bench", copy=_frames.ROWS)
    N, Fr = len(plan), len(src)
    windows = src.whole()
    o_place = Fr * 5 + (Fr * 5) % 2
    o_holes = o_place + N * augment.MAX_PLACE * 12
    o_np = o_holes + N * augment.MAX_HOLES * 2
    buf = _gather.pack_records(windows, *src.records(windows), tail_words=o_np + (N + 1) // 2 - Fr * 5)
    plan.pack(buf[o_place:o_holes].view(np.int32).reshape(-1, 24), buf[o_holes:o_np].view(np.int32).reshape(-1, 4), buf[o_np:].view(np.int32)[:N])
    d = torch.from_numpy(buf).cuda()
    canvas = torch.empty((N, plan.height, plan.width, 3), dtype=torch.uint8, device="cuda")
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    word, hole_word = _frames.fill_word(fill, 3), _frames.fill_word(hole_fill, 3)

    def fn():
        _lib.check(lib.cnl_augment_u8(d.data_ptr(), Fr, d[o_place:].data_ptr(), d[o_np:].data_ptr(), plan.max_place, d[o_holes:].data_ptr(),
                                      canvas.data_ptr(), N, plan.height, plan.width, word, hole_word, stream), "cnl_augment_u8")
    fn.keep = (src, d)
    return fn, canvas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("augment_bench needs a HIP device: nothing is measured without one")
    lines = [f"command: python tools/augment_bench.py --calls {args.calls}", "device: " + torch.cuda.get_device_name(0)]
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device="cuda") for (h, w) in sizes]
    targets = make_targets(sizes, 1)
    fill, hole_fill = (114, 114, 114), (0, 0, 0)
    lines.append(f"workload: 16 x 1080x1920 + 16 x 720x1280 RGB frames, {BOXES} boxes each -> 32 canvases; settings {SETTINGS}; per call, the median "
                 f"of {args.calls} calls, variants alternating")
    for (H, W) in ((512, 512), (608, 1088)):
        for mosaic in (0.0, 1.0):
            plan = cl.sample_augment(sizes, H, W, np.random.default_rng(2), mosaic=mosaic, **SETTINGS)
            alone, alone_canvas = kernel_alone(frames, plan, fill, hole_fill)
            variants = [("(a) augment_batch (upload + 2 launches)", lambda: cl.augment_batch(frames, plan, targets, fill=fill, hole_fill=hole_fill)),
                        ("(b) torch ops, per image", lambda: torch_baseline(frames, plan, targets, fill, hole_fill)),
                        ("(c) cnl_augment_u8 alone", alone)]
            a, b = variants[0][1](), variants[1][1]()
            alone()
            torch.cuda.synchronize()
            assert torch.equal(a[0], alone_canvas), "the call and the entry alone disagree"
            diff = (a[0].int() - b[0].int()).abs()
            same_count = bool(torch.equal(a[1]["count"], b[1]["count"]))
            for _, fn in variants:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = [[] for _ in variants]
            for _ in range(args.calls):
                for i, (_, fn) in enumerate(variants):
                    t[i].append(call_ms(fn))
            med = [float(np.median(v)) for v in t]
            moved = must_move_bytes(plan)
            lines.append(f"--- {H} x {W}, mosaic {mosaic:g}: {int(plan.n_place.sum())} placements, {int(a[1]['count'].sum())} of "
                         f"{int(plan.n_place.sum()) * BOXES} boxes kept (torch ops keep the same counts: {same_count}; canvas differs from theirs by "
                         f"at most {int(diff.max())}, mean {float(diff.float().mean()):.3f}: another interpolation rule)")
            for (name, _), v, m in zip(variants, t, med):
                lines.append(f"{name:<42} : median {m * 1e3:10.1f} us   min {min(v) * 1e3:.1f}  max {max(v) * 1e3:.1f}")
            lines.append(f"(b) / (a): {med[1] / med[0]:.1f} x;  (c) must-move bytes {moved / 1e6:.1f} MB -> {moved / (med[2] * 1e-3) / 1e12:.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
