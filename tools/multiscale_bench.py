"""Times the multi-scale test and writes profiles/multiscale_bench.txt:
  (a) the soft merge alone (merge_soft: the sort stage + one workgroup per frame) at N = 32 frames, S = 5 scales, k = 100 detections per
      view, for its three methods, beside merge_tiles (the hard merge, three kernels) on the same candidates and beside the numpy
      restatement of the rule (tests/soft_nms_ref.soft_merge_ref) on the host, the detections downloaded first (a host clock around the
      download and the loop).  The candidates are planted objects with jittered duplicates (soft_nms_ref.planted_candidates): crowded,
      as a multi-scale pass is; each GPU result is checked against the restatement before it is timed.
  (b) detect_multiscale on 32 frames of 480 x 640 with the defaults (five scales of a 512 x 512 canvas) against the sum of five
      detect_frames calls at the same canvases, and merge_soft on detect_multiscale's own detections: the merge's share of the step.
p50 of device-event times over --reps repetitions after warm-up; the host enqueues inside the window.

    python tools/multiscale_bench.py [--reps 20] [--out profiles/multiscale_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import soft_nms_ref as ref  # noqa: E402
import centernet_lightning_amd as cl  # noqa: E402


def p50_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def host_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiscale_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multiscale_bench.py needs a HIP device"
    N, S, k = args.frames, 5, 100
    kw = dict(sigma=0.5, iou_threshold=0.5, score_threshold=0.05, max_detections=100, class_aware=True, max_candidates=4096)

    # ---- (a) the merge alone, on planted candidates
    rec, ffv = ref.scale_records([ref.FRAME_SIZES[n % 3] for n in range(N)], S)
    boxes, scores, labels = ref.planted_candidates(np.random.default_rng(2024), rec, ffv, k)
    geom = cl.TileGeometry.from_records(rec, ffv, "cuda")
    dev = [torch.from_numpy(a).cuda() for a in (boxes, scores, labels)]
    ref_kw = {key: v for key, v in kw.items() if key != "max_detections"}
    rows, counts = [], {}
    for method in ("hard", "linear", "gaussian"):
        got = cl.merge_soft(*dev, geom, method=method, **kw)
        want = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 100, method=method, **ref_kw)
        for key in ("count", "source", "labels"):
            assert np.array_equal(got[key].cpu().numpy(), want[key]), f"merge_soft {method} differs from the restatement in {key}"
        assert np.abs(got["scores"].cpu().numpy() - want["scores"]).max() <= (2.0 ** -24 if method == "gaussian" else 0.0)
        counts[method] = (int(want["count"].min()), int(want["count"].max()))
        rows.append((f"merge_soft {method} (sort stage + one workgroup per frame)", p50_ms(lambda: cl.merge_soft(*dev, geom, method=method, **kw), args.reps)))

        def on_the_host(method=method):
            b, s, l = (t.cpu().numpy() for t in dev)
            ref.soft_merge_ref(b, s, l, rec, ffv, 100, method=method, **ref_kw)
        rows.append((f"the numpy restatement of {method} on the host, detections downloaded first", host_ms(on_the_host, args.host_reps)))
    hard_kw = dict(max_detections=100, score_threshold=0.05, match_threshold=0.5, match_metric="iou", class_aware=True, max_candidates=4096)
    rows.append(("merge_tiles (the hard merge: three kernels) on the same candidates", p50_ms(lambda: cl.merge_tiles(*dev, geom, **hard_kw), args.reps)))
    passing = int((scores > np.float32(0.05)).sum())

    # ---- (b) the whole step
    model = bench.build_model("simple")
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(N)]
    sizes = cl.multiscale_sizes(512, 512, ref.SCALES)
    multi = model.detect_multiscale(frames)
    t_multi = p50_ms(lambda: model.detect_multiscale(frames), args.reps)
    t_frames = [p50_ms(lambda: model.detect_frames(frames, h, w), args.reps) for (h, w) in sizes]
    # merge_soft on the detections detect_multiscale itself merges
    dets, views = model._detect_scales(frames, sizes)
    own = cl.merge_soft(dets["bboxes"], dets["scores"], dets["labels"], views)
    assert torch.equal(own["scores"], multi["scores"]) and torch.equal(own["bboxes"], multi["bboxes"])
    t_own = p50_ms(lambda: cl.merge_soft(dets["bboxes"], dets["scores"], dets["labels"], views), args.reps)
    sum_frames = sum(t[0] for t in t_frames)

    lines = [f"multiscale_bench (a): {N} frames x {S} scales x {k} detections, planted objects with jittered duplicates; {passing} of {N * S * k} candidates "
             f"above 0.05; picks per frame: " + ", ".join(f"{m} {lo}..{hi}" for m, (lo, hi) in counts.items()),
             f"device-event times in ms, p50 (min .. max) over {args.reps} repetitions after warm-up (host clock, {args.host_reps} repetitions, for the "
             f"numpy rows); the host enqueues inside the window", ""]
    for name, t in rows:
        lines.append(f"  {name:<84s} {t[0]:10.3f}  ({t[1]:.3f} .. {t[2]:.3f})")
    lines += ["", f"multiscale_bench (b): {N} frames of 480 x 640, resnet34_simple with synthetic weights, canvases " + ", ".join(f"{h} x {w}" for h, w in sizes)
              + f"; picks per frame {int(multi['count'].min())}..{int(multi['count'].max())}", ""]
    rows_b = [("detect_multiscale, whole (five letterboxes, forwards and decodes, one merge)", t_multi)]
    rows_b += [(f"detect_frames at {h} x {w}", t) for (h, w), t in zip(sizes, t_frames)]
    rows_b += [("merge_soft gaussian on detect_multiscale's own detections", t_own)]
    for name, t in rows_b:
        lines.append(f"  {name:<84s} {t[0]:10.3f}  ({t[1]:.3f} .. {t[2]:.3f})")
    lines += ["", f"sum of the five detect_frames p50 = {sum_frames:.3f} ms; detect_multiscale / that sum = {t_multi[0] / sum_frames:.4f}; "
                  f"the merge's share of the step = merge_soft / detect_multiscale = {t_own[0] / t_multi[0]:.4f} (p50 over p50)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
