"""Times sliced inference on 32 frames of 1080 x 1920 with the defaults (512 x 512 tiles, overlap 0.2, the full-frame view: 512 views,
16 chunks of 32) and writes profiles/tiled_bench.txt: the tile gather launch, the merge (its three kernels), the whole detect_tiled,
and beside them two baselines that are not the code under test:
  (i)  the same merge rule written with plain torch ops on the device, looped per frame (checked equal to tests/tiled_ref.merge_ref
       and to the HIP merge before it is timed);
  (ii) forward_uint8 + gather_detection2d on the same 512 views: the work the merge sits behind.
p50 of device-event times over --reps repetitions after warm-up (the torch baseline over --torch-reps: it takes seconds).

    python tools/tiled_bench.py [--reps 20] [--out profiles/tiled_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import tiled_ref  # noqa: E402
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


def torch_merge(boxes, scores, labels, records, ffv, K, score_threshold, match_threshold, metric, class_aware, cap):
    """Baseline (i): rules 1-6 with torch ops, one frame at a time; every op is its own kernel, so every operation rounds once."""
    dev = boxes.device
    rec = torch.tensor([[float(x) for x in r] for r in records], dtype=torch.float32, device=dev)
    N, k = len(ffv) - 1, boxes.shape[1]
    out_b = torch.zeros((N, K + 1, 4), device=dev)
    out_s = torch.zeros((N, K + 1), device=dev)
    out_l = torch.zeros((N, K + 1), dtype=torch.int64, device=dev)
    out_c = torch.full((N, K + 1), -1, dtype=torch.int32, device=dev)
    count = torch.zeros((N,), dtype=torch.int32, device=dev)
    zero = torch.zeros((), device=dev)
    score_threshold = torch.tensor(score_threshold, dtype=torch.float32, device=dev)
    match_threshold = torch.tensor(match_threshold, dtype=torch.float32, device=dev)
    for n in range(N):
        v0, v1 = ffv[n], ffv[n + 1]
        r = rec[v0:v1, None, :]
        b = boxes[v0:v1]
        cols = []
        for c, (pad, s, o, lim) in enumerate(((4, 6, 2, 0), (5, 7, 3, 1), (4, 6, 2, 0), (5, 7, 3, 1))):
            v = (b[..., c] - r[..., pad]) / r[..., s] + r[..., o]
            cols.append(torch.minimum(torch.maximum(v, zero), r[..., lim].expand_as(v)))
        mapped = torch.stack(cols, dim=-1).reshape(-1, 4)
        s, lab = scores[v0:v1].reshape(-1), labels[v0:v1].reshape(-1)
        valid = s > score_threshold
        order = torch.sort(torch.where(valid, s, torch.full_like(s, -float("inf"))), descending=True, stable=True).indices[:cap]
        m, sl, ll, ok = mapped[order], s[order], lab[order], valid[order]
        M = m.shape[0]
        x1, y1, x2, y2 = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
        iw = (torch.minimum(x2[:, None], x2[None, :]) - torch.maximum(x1[:, None], x1[None, :])).clamp_min(0)
        ih = (torch.minimum(y2[:, None], y2[None, :]) - torch.maximum(y1[:, None], y1[None, :])).clamp_min(0)
        inter = iw * ih
        area = (x2 - x1) * (y2 - y1)
        denom = torch.minimum(area[:, None], area[None, :]) if metric == 1 else (area[:, None] + area[None, :]) - inter
        hit = (inter > match_threshold * denom).triu(1)
        if class_aware:
            hit &= ll[:, None] == ll[None, :]
        removed = ~ok
        for i in range(M):
            removed = removed | (hit[i] & ~removed[i])
        kept = ~removed
        rank = torch.cumsum(kept, 0) - 1
        slot = torch.where(kept & (rank < K), rank, torch.full_like(rank, K))
        out_b[n].index_copy_(0, slot, m)
        out_s[n].index_copy_(0, slot, sl)
        out_l[n].index_copy_(0, slot, ll)
        out_c[n].index_copy_(0, slot, order.to(torch.int32))
        count[n] = kept.sum().clamp_max(K)
    pad = torch.arange(K, device=dev)[None, :] >= count[:, None]
    return {"bboxes": out_b[:, :K].masked_fill(pad[..., None], 0), "scores": out_s[:, :K].masked_fill(pad, 0),
            "labels": out_l[:, :K].masked_fill(pad, 0), "source": out_c[:, :K].masked_fill(pad, -1), "count": count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=7)
    ap.add_argument("--merge-only", type=int, default=0, metavar="R", help="after the set-up run merge_tiles R times and exit: the run to put under a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tiled_bench.py needs a HIP device"
    model = bench.build_model("simple")
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (1080, 1920, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(args.frames)]
    views, geom = cl.tile_uint8(frames)
    V = views.shape[0]

    def forward_and_decode():
        parts = [model._detect_views(views[i:i + 32], "tiled_bench", model.IMAGENET_MEAN, model.IMAGENET_STD, False, 100, 3) for i in range(0, V, 32)]
        return {key: torch.cat([p[key] for p in parts]) for key in parts[0]}

    dets = forward_and_decode()
    kw = dict(max_detections=300, score_threshold=0.1, match_threshold=0.5, match_metric="iou", class_aware=True, max_candidates=4096)
    merged = cl.merge_tiles(dets["bboxes"], dets["scores"], dets["labels"], geom, **kw)
    # the baseline is checked before it is timed: against the numpy rule on the first frames, against the HIP merge on all of them
    import letterbox_ref
    rec, ffv, _ = tiled_ref.view_records([(1080, 1920)] * args.frames, 512, 512, 0.2, True, letterbox_ref.geometry)
    base = torch_merge(dets["bboxes"], dets["scores"], dets["labels"], rec, ffv, 300, 0.1, 0.5, 0, True, 4096)
    d = {key: v.cpu().numpy() for key, v in dets.items()}
    want = tiled_ref.merge_ref(d["bboxes"][:ffv[2]], d["scores"][:ffv[2]], d["labels"][:ffv[2]], rec[:ffv[2]], ffv[:3], 300)
    for key in want:
        assert np.array_equal(base[key][:2].cpu().numpy(), want[key]), f"torch baseline differs from merge_ref in {key}"
        assert torch.equal(base[key], merged[key]), f"torch baseline differs from the HIP merge in {key}"
    passing = int((dets["scores"] > 0.1).sum())
    if args.merge_only:
        torch.cuda.synchronize()
        for _ in range(args.merge_only):
            cl.merge_tiles(dets["bboxes"], dets["scores"], dets["labels"], geom, **kw)
        torch.cuda.synchronize()
        print(f"merge_tiles ran {args.merge_only + 1} times ({passing} candidates above 0.1)")
        return

    t_gather = p50_ms(lambda: cl.tile_uint8(frames), args.reps)
    t_merge = p50_ms(lambda: cl.merge_tiles(dets["bboxes"], dets["scores"], dets["labels"], geom, **kw), args.reps)
    t_whole = p50_ms(lambda: model.detect_tiled(frames), args.reps)
    t_fwd = p50_ms(forward_and_decode, args.reps)
    t_torch = p50_ms(lambda: torch_merge(dets["bboxes"], dets["scores"], dets["labels"], rec, ffv, 300, 0.1, 0.5, 0, True, 4096), args.torch_reps, warmup=1)
    lines = [f"tiled_bench: {args.frames} frames of 1080 x 1920, tiles 512 x 512, overlap 0.2, full-frame view: {V} views, chunks of 32; "
             f"{passing} of {V * 100} candidates above 0.1, merged counts {int(merged['count'].min())}..{int(merged['count'].max())} per frame",
             f"device-event times in ms, p50 (min .. max) over {args.reps} repetitions after warm-up ({args.torch_reps} for the torch baseline); "
             f"the host enqueues inside the window", ""]
    for name, t in (("tile gather (tile_uint8: table upload + ONE launch)", t_gather), ("merge (merge_tiles: three kernels)", t_merge),
                    ("detect_tiled, whole", t_whole), ("baseline (ii): forward_uint8 + gather_detection2d on the same views", t_fwd),
                    ("baseline (i): the merge rule in torch ops, per frame", t_torch)):
        lines.append(f"  {name:<72s} {t[0]:10.3f}  ({t[1]:.3f} .. {t[2]:.3f})")
    lines += ["", f"merge / baseline (ii) = {t_merge[0] / t_fwd[0]:.4f} (p50 of {args.reps} over p50 of {args.reps}); "
                  f"merge / baseline (i) = {t_merge[0] / t_torch[0]:.5f} (p50 of {args.reps} over p50 of {args.torch_reps})",
              "the windows include the host's enqueue work (tensor allocation, the ctypes call): the kernels alone are in the kernel trace below"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
