"""Affine augmentation micro-benchmark: 32 mixed 1080p / 720p RGB frames with 40 boxes each -> 32 canvases of 512 x 512 and of 608 x 1088
with the MOT config's settings (HorizontalFlip 0.5, Affine scale [0.8, 1.25] rotate [-10, 10], RandomResizedCrop, ColorJitter
0.4 / 0.4 / 0.4, Cutout 10 x 60 x 60).

  (a) warp_batch: the one call (one pinned upload: frame records + plan; cnl_augment_warp_u8 + cnl_augment_warp_boxes_f64)
  (b) cnl_augment_warp_u8 alone on that plan (prebuilt device records, no upload)
  (c) an AXIS-ALIGNED plan (sample_augment's windows and flips, no rotation) on the same canvases, three ways: cnl_augment_warp_u8 on the
      plan written as affine maps; cnl_augment_u8 of this library; cnl_augment_u8 of the PARENT commit's library (--parent-lib: a
      libcenternet_gfx950.so built from the commit before the warp kernel; left out when not given).  What a rotated gather costs
      against the table-driven separable one, and whether sharing augment.hip's colour step and holes through a header moved it.
  (d) a per-image torch loop on the plan of (a): F.affine_grid + F.grid_sample (bilinear, zeros padding: NOT the same bytes), the colour
      matrix as a matmul, hole fills.  What a user writes without (a); pixels only.

Per call: device events around ONE call, the median of --calls calls (>= 20), after a warm-up of every variant, the variants alternating.
No bar: nothing gates on these figures.

    python tools/warp_bench.py [--calls 20] [--parent-lib PATH] [--out profiles/warp_bench.txt]"""
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
from centernet_lightning_amd import _frames, _gather, _lib, augment, warp        # noqa: E402

JITTER = dict(flip=0.5, brightness=0.4, contrast=0.4, saturation=0.4, cutout=(10, 60, 60))
MOT = dict(affine_scale=(0.8, 1.25), rotate=(-10, 10), **JITTER)
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


def as_warp_plan(plan):
    """An AugmentPlan as the WarpPlan that samples the same windows into the same rectangles (the clip window is the plan's window)."""
    out = cl.WarpPlan.empty(plan.sizes, plan.height, plan.width, N=len(plan))
    out.n_place, out.frame, out.window, out.dest, out.colour, out.holes = plan.n_place, plan.frame, plan.window, plan.dest, plan.colour, plan.holes
    for n in range(len(plan)):
        for p in range(int(plan.n_place[n])):
            x0, y0, w, h = (int(v) for v in plan.window[n, p])
            _, _, dw, dh = (int(v) for v in plan.dest[n, p])
            sx, sy = dw / w, dh / h
            fwd = [sx, 0.0, -x0 * sx, 0.0, sy, -y0 * sy]
            if plan.flip[n, p]:
                fwd[0], fwd[2] = -fwd[0], dw - fwd[2]
            out.set_map(n, p, fwd)
    return out.check()


def kernel_alone(lib, entry, frames, plan, words):
    """-> (fn, canvas): the image entry `entry` of `lib` on records uploaded once."""
    src = _frames.open_frames(frames, "rgb", "warp_bench", copy=_frames.ROWS)
    N, Fr = len(plan), len(src)
    record_words = warp.RECORD_WORDS if isinstance(plan, cl.WarpPlan) else 12
    windows = src.whole()
    o_place = Fr * 5 + (Fr * 5) % 2
    o_holes = o_place + N * augment.MAX_PLACE * record_words
    o_np = o_holes + N * augment.MAX_HOLES * 2
    buf = _gather.pack_records(windows, *src.records(windows), tail_words=o_np + (N + 1) // 2 - Fr * 5)
    plan.pack(buf[o_place:o_holes].view(np.int32).reshape(-1, 2 * record_words), buf[o_holes:o_np].view(np.int32).reshape(-1, 4), buf[o_np:].view(np.int32)[:N])
    d = torch.from_numpy(buf).cuda()
    canvas = torch.empty((N, plan.height, plan.width, 3), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = getattr(lib, entry)

    def fn():
        rc = call(d.data_ptr(), Fr, d[o_place:].data_ptr(), d[o_np:].data_ptr(), plan.max_place, d[o_holes:].data_ptr(), canvas.data_ptr(), N, plan.height,
                  plan.width, *words, stream)
        assert rc == 0, (entry, rc)
    fn.keep = (src, d)
    return fn, canvas


def load_parent(path):
    lib = ctypes.CDLL(path)
    lib.cnl_augment_u8.restype, lib.cnl_augment_u8.argtypes = _lib._SIGNATURES["cnl_augment_u8"]
    return lib


def torch_baseline(frames, plan, fill, hole_fill, border):
    """The plan's pixels with torch ops, one image and one placement at a time: the inverse map as an affine_grid theta (normalised
    coordinates, align_corners=False), grid_sample (bilinear; zeros padding stands in for the border colour), the colour matrix, the holes."""
    N, H, W = len(plan), plan.height, plan.width
    canvas = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    canvas[...] = torch.tensor(fill, dtype=torch.uint8, device="cuda")
    for n in range(N):
        for p in range(int(plan.n_place[n])):
            f = int(plan.frame[n, p])
            fh, fw = plan.sizes[f]
            dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
            A = np.linalg.inv(np.vstack([plan.fwd[n, p].reshape(2, 3), [0, 0, 1]]))           # rectangle coordinates -> frame coordinates
            to_unit = np.array([[2 / fw, 0, -1], [0, 2 / fh, -1], [0, 0, 1]])
            from_unit = np.array([[dw / 2, 0, dw / 2], [0, dh / 2, dh / 2], [0, 0, 1]])
            theta = torch.from_numpy((to_unit @ A @ from_unit)[:2]).float().cuda()[None]
            grid = F.affine_grid(theta, (1, 3, dh, dw), align_corners=False)
            r = F.grid_sample(frames[f].permute(2, 0, 1)[None].float(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0].permute(1, 2, 0)
            q = torch.from_numpy(plan.colour[n, p].astype(np.float32) / 4096.0).cuda()
            r = r @ q[:9].view(3, 3).T + q[9:]
            canvas[n, dy0:dy0 + dh, dx0:dx0 + dw] = r.round().clamp(0, 255).to(torch.uint8)
        for (hx, hy, hw, hh) in plan.holes[n].tolist():
            if hw > 0 and hh > 0:
                canvas[n, max(hy, 0):max(min(hy + hh, H), 0), max(hx, 0):max(min(hx + hw, W), 0)] = torch.tensor(hole_fill, dtype=torch.uint8, device="cuda")
    return canvas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libcenternet_gfx950.so built from the parent commit, for row (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("warp_bench needs a HIP device: nothing is measured without one")
    lib = _lib.load()
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    lines = [f"command: python tools/warp_bench.py --calls {args.calls}" + (" --parent-lib <the parent commit's library>" if parent else ""),
             "device: " + torch.cuda.get_device_name(0)]
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device="cuda") for (h, w) in sizes]
    targets = make_targets(sizes, 1)
    fill, hole_fill, border = (114, 114, 114), (0, 0, 0), (0, 0, 0)
    words = [_frames.fill_word(c, 3) for c in (fill, hole_fill, border)]
    lines.append(f"workload: 16 x 1080x1920 + 16 x 720x1280 RGB frames, {BOXES} boxes each -> 32 canvases; settings {MOT}; per call, the median of "
                 f"{args.calls} calls, variants alternating")
    for (H, W) in ((512, 512), (608, 1088)):
        plan = cl.sample_warp(sizes, H, W, np.random.default_rng(2), **MOT)
        aligned = cl.sample_augment(sizes, H, W, np.random.default_rng(2), **JITTER)
        aligned_warp = as_warp_plan(aligned)
        alone, alone_canvas = kernel_alone(lib, "cnl_augment_warp_u8", frames, plan, words)
        c_warp, c_warp_canvas = kernel_alone(lib, "cnl_augment_warp_u8", frames, aligned_warp, words)
        c_this, c_this_canvas = kernel_alone(lib, "cnl_augment_u8", frames, aligned, words[:2])
        variants = [("(a) warp_batch (upload + 2 launches)", lambda: cl.warp_batch(frames, plan, targets, fill=fill, hole_fill=hole_fill, border=border)),
                    ("(b) cnl_augment_warp_u8 alone", alone),
                    ("(c) axis-aligned: cnl_augment_warp_u8", c_warp),
                    ("(c) axis-aligned: cnl_augment_u8", c_this)]
        if parent is not None:
            c_parent, c_parent_canvas = kernel_alone(parent, "cnl_augment_u8", frames, aligned, words[:2])
            variants.append(("(c) axis-aligned: cnl_augment_u8, parent", c_parent))
        variants.append(("(d) affine_grid + grid_sample, per image", lambda: torch_baseline(frames, plan, fill, hole_fill, border)))
        results = [fn() for _, fn in variants]
        torch.cuda.synchronize()
        assert torch.equal(results[0][0], alone_canvas), "the call and the entry alone disagree"
        if parent is not None:
            assert torch.equal(c_this_canvas, c_parent_canvas), "cnl_augment_u8 no longer writes the parent's bytes"
        rules = (c_warp_canvas.int() - c_this_canvas.int()).abs()
        diff = (results[0][0].int() - results[-1].int()).abs()
        for _, fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = [[] for _ in variants]
        for _ in range(args.calls):
            for i, (_, fn) in enumerate(variants):
                t[i].append(call_ms(fn))
        med = [float(np.median(v)) for v in t]
        lines.append(f"--- {H} x {W}: {int(plan.n_place.sum())} placements, {int(results[0][1]['count'].sum())} of {int(plan.n_place.sum()) * BOXES} boxes kept; "
                     f"canvas differs from (d)'s by at most {int(diff.max())}, mean {float(diff.float().mean()):.3f} (another interpolation rule); on the "
                     f"axis-aligned plan the two rules differ by at most {int(rules.max())}, mean {float(rules.float().mean()):.3f}"
                     + ("; cnl_augment_u8 writes the parent's bytes" if parent is not None else ""))
        for (name, _), v, m in zip(variants, t, med):
            lines.append(f"{name:<42} : median {m * 1e3:10.1f} us   min {min(v) * 1e3:.1f}  max {max(v) * 1e3:.1f}")
        lines.append(f"(d) / (a): {med[-1] / med[0]:.1f} x;  warp / separable kernel on the axis-aligned plan: {med[2] / med[3]:.2f} x"
                     + (f";  cnl_augment_u8 / parent's: {med[3] / med[4]:.2f} x" if parent is not None else ""))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
