"""Times MotEvaluator (csrc/mot_eval.hip) on a synthetic MOT17-train-sized evaluation and compares it with the numpy + scipy restatement
of the same rule (tests/mot_eval_ref.py) run on the host over a subset.  TrackEval is not available to time; the restatement walks
pairs in plain Python where TrackEval uses numpy, so its time is an upper bound on "host evaluation", not a measurement of it.

    python tools/mot_eval_bench.py [--sequences 7] [--frames 1000] [--objects 30] [--ref-sequences 1] [--ref-frames 200] [--out profiles/mot_eval_bench.txt]

7 sequences x 1000 frames; --objects 30 gives a world of 60 pedestrians per sequence of which about 24 are in view at a time.  update() only collects on the host; get_metrics() is timed whole
(relabelling and pooling on the host, one upload, the launches, one download, the host fields), and its host pooling part alone.  The
restatement runs over the first --ref-frames frames of the first --ref-sequences sequences, and the evaluator over the same subset must
agree with it bit for bit, or the tool fails.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import centernet_lightning_amd as cl  # noqa: E402
from centernet_lightning_amd import mot_eval  # noqa: E402
import mot_eval_ref as ref  # noqa: E402


def synthetic_sequence(frames, objects, seed):
    """A world of 2 * objects pedestrians that walk through a 1920 x 1080 frame, each visible for a window of the sequence (about
    0.8 * `objects` at a time); the tracker finds one with probability 0.9 as a jittered box, loses its identity now and then, and adds
    false positives under 40 recurring ids."""
    rng = np.random.default_rng(seed)
    world = 2 * objects
    first = rng.integers(-frames // 2, frames, world)
    last = first + rng.integers(frames // 4, frames, world)
    pos, vel = rng.uniform([0, 0], [1920, 1080], (world, 2)), rng.normal(0, 2, (world, 2))
    wh = np.exp(rng.uniform(np.log(20), np.log(200), (world, 1))) * np.array([[0.4, 1.0]])
    trk, next_trk, out = np.arange(world) + 1000, 5000, []
    for f in range(frames):
        vis = np.flatnonzero((first <= f) & (f < last))
        gt = np.concatenate([pos[vis], wh[vis]], 1)
        found = vis[rng.random(len(vis)) < 0.9]
        for g in found[rng.random(len(found)) < 0.01]:
            trk[g], next_trk = next_trk, next_trk + 1
        pred = np.concatenate([pos[found] + rng.normal(0, 3, (len(found), 2)), wh[found] * (1 + rng.normal(0, 0.05, (len(found), 2)))], 1)
        n_fp = int(rng.integers(0, 4))
        clutter = np.concatenate([rng.uniform([0, 0], [1920, 1080], (n_fp, 2)), np.exp(rng.uniform(np.log(20), np.log(200), (n_fp, 2)))], 1)
        out.append((gt, vis + 1, np.concatenate([pred, clutter]), np.concatenate([trk[found], 900000 + rng.permutation(40)[:n_fp]])))
        pos = pos + vel
    return out


def fill(ev, sequences):
    for name, frames in sequences.items():
        ev.update([f[2] for f in frames], [f[3] for f in frames], [f[0] for f in frames], [f[1] for f in frames], sequence=name)


def same(got, want):
    for name, w in want.items():
        for key, v in w.items():
            g = got[name][key]
            if not (np.asarray(g).tobytes() == np.asarray(v).tobytes() if isinstance(v, np.ndarray) else (g == v and type(g) is type(v))):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=7)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--ref-sequences", type=int, default=1)
    ap.add_argument("--ref-frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mot_eval_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    sequences = {f"seq_{s}": synthetic_sequence(a.frames, a.objects, s) for s in range(a.sequences)}
    n_gt = sum(len(f[1]) for fr in sequences.values() for f in fr)
    n_pr = sum(len(f[3]) for fr in sequences.values() for f in fr)

    warm = cl.MotEvaluator()
    fill(warm, {"w": sequences["seq_0"][:20]})
    warm.get_metrics()                                          # library load, allocator, the kernels' first launch
    ev = cl.MotEvaluator()
    t0 = time.perf_counter()
    fill(ev, sequences)
    update_ms = (time.perf_counter() - t0) * 1e3
    total_ms, pool_ms = [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics = ev.get_metrics()
        total_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        arrays, scalars, facts = mot_eval.pool(list(ev._sequences.items()))
        pool_ms.append((time.perf_counter() - t0) * 1e3)

    sub = {name: frames[:a.ref_frames] for name, frames in list(sequences.items())[:a.ref_sequences]}
    t0 = time.perf_counter()
    want = ref.evaluate(sub)
    ref_s = time.perf_counter() - t0
    sub_ev = cl.MotEvaluator()
    fill(sub_ev, sub)
    equal = same(sub_ev.get_metrics(), want)
    ref_frames = sum(len(f) for f in sub.values())

    c = metrics["COMBINED_SEQ"]
    lines = [
        f"mot_eval_bench: {a.sequences} sequences x {a.frames} frames, {n_gt / (a.sequences * a.frames):.1f} ground truths and "
        f"{n_pr / (a.sequences * a.frames):.1f} predictions per frame, ids per sequence: "
        + ", ".join(f"{f['G']} + {f['T']}" for f in facts),
        f"device: {torch.cuda.get_device_name(0)}",
        f"update (host only: checks and copies), all {a.sequences * a.frames} frames: {update_ms:.1f} ms",
        f"get_metrics, whole (pooling, one upload, the launches, one download, host fields), {a.repeats} calls: median {np.median(total_ms):.1f} ms, "
        f"min {np.min(total_ms):.1f} ms, max {np.max(total_ms):.1f} ms",
        f"  of which relabelling and pooling on the host: median {np.median(pool_ms):.1f} ms",
        f"  pooled sizes: {scalars['sim_total']} similarities, {scalars['pair_total']} id pairs, {scalars['id_total']} Identity matrix entries",
        f"numpy + scipy restatement (tests/mot_eval_ref.py, plain Python) on {ref_frames} frames: {ref_s:.2f} s "
        f"(about {ref_s * a.sequences * a.frames / ref_frames:.0f} s for all {a.sequences * a.frames} if linear in the frames); TrackEval is not available to time",
        f"evaluator == restatement on those {ref_frames} frames, bit for bit: {equal}",
        f"COMBINED_SEQ of the synthetic data: HOTA {c['summary']['HOTA']:.4f}, DetA {c['summary']['DetA']:.4f}, AssA {c['summary']['AssA']:.4f}, "
        f"MOTA {c['MOTA']:.4f}, MOTP {c['MOTP']:.4f}, IDF1 {c['IDF1']:.4f}, IDSW {c['IDSW']}, Frag {c['Frag']}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not equal:
        sys.exit("the evaluator disagrees with the restatement")


if __name__ == "__main__":
    main()
