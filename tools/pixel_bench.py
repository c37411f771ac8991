"""Pixel-level augmentation micro-benchmark: 32 canvases of 512 x 512 and of 608 x 1088 (what cnl_augment_warp_u8 wrote from 32 mixed 1080p /
720p frames under the MOT config's settings, holes included) through three plans: all-MotionBlur (k = 15, lines drawn as MotionBlur draws
them), all-Equalize, and TrivialAugmentWide's mix (its photometric members with probability 1 / 13 each, every other canvas copied).

  (a) pixel_batch: the one call (one pinned upload: records + holes; a workspace; cnl_augment_pixel_u8's launches)
  (b) cnl_augment_pixel_u8 alone on that plan (prebuilt device records and workspace, no upload)
  (c) a per-canvas torch loop: F.conv2d with the tap kernel on a reflect-padded canvas; torch.bincount plus a gather for Equalize; the
      tables of Posterize / Solarize; hole fills.  What a user writes without (a).
  the launches: cnl_augment_pixel_u8 with a narrower `launches` word on the same records — 0: the apply launch alone (every canvas copied);
      HAS_TABLE: table + apply (Equalize gets the identity table: the same apply work); both: histogram + table + apply.  A launch's own
      time is the difference of two rows; each row is device events around one call.
  cnl_augment_warp_u8 alone on the plan that made the canvases, timed in the same loop: what the geometric pass costs beside it.

Per call: device events around ONE call, the median of --calls calls (>= 20), after a warm-up of every variant, the variants alternating.
No bar: nothing gates on these figures.

    python tools/pixel_bench.py [--calls 20] [--out profiles/pixel_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import centernet_lightning_amd as cl                       # noqa: E402
from centernet_lightning_amd import _frames, _lib, pixel   # noqa: E402
from warp_bench import MOT, call_ms, kernel_alone          # noqa: E402


def plans(N, rng):
    blur = cl.PixelPlan.empty(N)
    for n in range(N):
        pixel._draw_motion_blur(blur, n, rng, [15])
    equalize = cl.PixelPlan.empty(N)
    for n in range(N):
        equalize.set_equalize(n)
    mix = cl.PixelPlan.empty(N)
    members = [pixel.TRIVIAL_MEMBERS[n % 13] if n % 13 < 12 else None for n in rng.permutation(N)]      # every member equally often, as 12 / 13 draws them
    for n, m in enumerate(members):
        if m == "sharpen":
            mix.set_sharpen(n, float(rng.uniform(0.0, 0.99)))
        elif m == "posterize":
            mix.set_posterize(n, int(rng.integers(2, 9)))
        elif m == "solarize":
            mix.set_solarize(n, int(rng.integers(0, 256)))
        elif m == "equalize":
            mix.set_equalize(n)
    return [("all-MotionBlur k = 15", blur.check()), ("all-Equalize", equalize.check()), ("TrivialAugmentWide mix", mix.check())]


def entry_alone(lib, canvas, plan, holes, word, launches=None):
    """-> (fn, out): cnl_augment_pixel_u8 on records, holes and a workspace that are on the device already."""
    N, H, W = (int(v) for v in canvas.shape[:3])
    records = np.zeros((N, 2 * pixel.RECORD_WORDS), np.int32)
    plan.pack(records)
    d_ops, d_holes = torch.from_numpy(records).cuda(), torch.from_numpy(np.ascontiguousarray(holes)).cuda()
    need = int(lib.cnl_augment_pixel_workspace_bytes(N, H, W))
    space, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.empty_like(canvas)
    launches = plan.launches if launches is None else launches
    stream = _lib.stream(canvas.device)

    def fn():
        rc = lib.cnl_augment_pixel_u8(canvas.data_ptr(), N, H, W, d_ops.data_ptr(), launches, d_holes.data_ptr(), word, out.data_ptr(), space.data_ptr(), need,
                                      stream)
        assert rc == 0, rc
    fn.keep = (d_ops, d_holes, space)
    return fn, out


def torch_baseline(canvas, plan, holes, hole_fill):
    N, H, W = (int(v) for v in canvas.shape[:3])
    out = torch.empty_like(canvas)
    values = torch.arange(256, device="cuda")
    for n in range(N):
        op, img = int(plan.op[n]), canvas[n]
        if op == pixel.FILTER:
            taps = plan.taps[n, :int(plan.n_taps[n])]
            r = int(np.abs(taps[:, :2]).max())
            k = torch.zeros((2 * r + 1, 2 * r + 1))
            for dx, dy, w in taps.tolist():
                k[dy + r, dx + r] = w / 65536.0
            x = F.pad(img.permute(2, 0, 1)[None].float(), (r, r, r, r), mode="reflect") if r else img.permute(2, 0, 1)[None].float()
            y = F.conv2d(x, k.cuda().expand(3, 1, -1, -1).contiguous(), groups=3)[0].permute(1, 2, 0)
            res = y.round().clamp(0, 255).to(torch.uint8)
        elif op == pixel.POSTERIZE:
            res = img & ((0xFF << (8 - int(plan.param[n]))) & 0xFF)
        elif op == pixel.SOLARIZE:
            res = torch.where(img >= int(plan.param[n]), 255 - img, img)
        elif op == pixel.EQUALIZE:
            res = torch.empty_like(img)
            for c in range(3):
                ch = img[..., c].long()
                h = torch.bincount(ch.reshape(-1), minlength=256)
                i0 = (h > 0).int().argmax()
                d = H * W - h[i0]
                cum = torch.cumsum(h, 0) - torch.cumsum(h, 0)[i0]
                lut = torch.where(values <= i0, torch.zeros_like(values), (510 * cum + d) // (2 * d).clamp(min=1))
                lut = torch.where(d > 0, lut, values)
                res[..., c] = lut[ch].to(torch.uint8)
        else:
            res = img
        out[n] = res
        for (hx, hy, hw, hh) in holes[n].tolist():
            if hw > 0 and hh > 0:
                out[n, max(hy, 0):max(min(hy + hh, H), 0), max(hx, 0):max(min(hx + hw, W), 0)] = torch.tensor(hole_fill, dtype=torch.uint8, device="cuda")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("pixel_bench needs a HIP device: nothing is measured without one")
    lib = _lib.load()
    lines = [f"command: python tools/pixel_bench.py --calls {args.calls}", "device: " + torch.cuda.get_device_name(0)]
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device="cuda") for (h, w) in sizes]
    # smooth content, so that a histogram is not flat: a frame's noise over a gradient
    for f in frames:
        ramp = torch.linspace(0, 160, f.shape[1], device="cuda")[None, :, None]
        f.copy_((f.float() * 0.35 + ramp).clamp(0, 255).to(torch.uint8))
    fill, hole_fill, border = (114, 114, 114), (0, 0, 0), (0, 0, 0)
    words = [_frames.fill_word(c, 3) for c in (fill, hole_fill, border)]
    lines.append(f"workload: 32 canvases written by cnl_augment_warp_u8 from 16 x 1080x1920 + 16 x 720x1280 RGB frames (settings {MOT}), their holes punched "
                 f"by the pixel pass; per call, the median of {args.calls} calls, variants alternating")
    for (H, W) in ((512, 512), (608, 1088)):
        warp_plan = cl.sample_warp(sizes, H, W, np.random.default_rng(2), **MOT)
        holes = warp_plan.holes
        warp_plan.holes = np.zeros_like(holes)
        warp_alone, canvas = kernel_alone(lib, "cnl_augment_warp_u8", frames, warp_plan, words)
        warp_alone()
        torch.cuda.synchronize()
        N = len(warp_plan)
        lines.append(f"--- {H} x {W}: {N} canvases, {N * H * W * 3 / 1e6:.1f} MB read and as much written; workspace "
                     f"{lib.cnl_augment_pixel_workspace_bytes(N, H, W) / 1e6:.2f} MB")
        copy_alone, _ = entry_alone(lib, canvas, cl.PixelPlan.empty(N), holes, words[1])
        for name, plan in plans(N, np.random.default_rng(3)):
            alone, alone_out = entry_alone(lib, canvas, plan, holes, words[1])
            variants = [("(a) pixel_batch (upload + launches)", lambda plan=plan: cl.pixel_batch(canvas, plan, holes=holes, hole_fill=hole_fill)),
                        ("(b) cnl_augment_pixel_u8 alone", alone)]
            if plan.launches & pixel.HAS_EQUALIZE:
                variants.append(("    launches = HAS_TABLE: table + apply", entry_alone(lib, canvas, plan, holes, words[1], pixel.HAS_TABLE)[0]))
            variants += [("    launches = 0: apply alone, as a copy", copy_alone), ("cnl_augment_warp_u8 alone, same canvases", warp_alone),
                         ("(c) torch ops, per canvas", lambda plan=plan: torch_baseline(canvas, plan, holes, hole_fill))]
            results = [fn() for _, fn in variants]
            torch.cuda.synchronize()
            assert torch.equal(results[0], alone_out), "the call and the entry alone disagree"
            diff = (results[0].int() - results[-1].int()).abs()
            for _, fn in variants:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = [[] for _ in variants]
            for _ in range(args.calls):
                for i, (_, fn) in enumerate(variants):
                    t[i].append(call_ms(fn))
            med = [float(np.median(v)) for v in t]
            ops = np.bincount(plan.op, minlength=5).tolist()
            lines.append(f"{name}: canvases per operation (NONE, FILTER, POSTERIZE, SOLARIZE, EQUALIZE) {ops}; bytes differ from (c)'s in "
                         f"{int((diff > 0).sum())} of {diff.numel()}, by at most {int(diff.max())}")
            for (label, _), v, m in zip(variants, t, med):
                lines.append(f"  {label:<42} : median {m * 1e3:10.1f} us   min {min(v) * 1e3:.1f}  max {max(v) * 1e3:.1f}")
            lines.append(f"  (c) / (a): {med[-1] / med[0]:.1f} x;  (b) / warp kernel: {med[1] / med[-2]:.2f} x;  (b) moves "
                         f"{2 * N * H * W * 3 / med[1] / 1e6:.0f} GB/s of canvas bytes")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
