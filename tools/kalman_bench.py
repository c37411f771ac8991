"""Kalman filter measurement: what use_kalman=True costs a tracking step on the host path and on the device path.

    python tools/kalman_bench.py [--streams 32] [--steps 20] [--warmup 10] [--rows 70,2240,4480] [--package DIR]

In ONE process, step by step alternating between the variants on the same frames, each step closed by a device synchronisation, median
(p10, p90) of the wall time per step over `--steps` steps after `--warmup`:
  (a) TrackerBank.update_batch at S streams, k = 300 detections, ~58 kept, ~70 tracks per stream (the shapes of
      profiles/track_streams_bench.txt), with use_kalman=False / use_kalman=True, kalman="host" / kalman="device";
  (b) Tracker.update at one stream, the same three variants;
  (c) cnl_track_kalman_f64 alone at R rows (every row matched and predicted: the longest path), by HIP events, and launch + synchronisation
      as the host sees it with the record in mapped memory.
`--package DIR` imports centernet_lightning_amd from DIR (a checkout of another commit's centernet-lightning_amd/, with CENTERNET_GFX950_LIB
naming a built library) instead of this tree: the host path's cost AT THE PARENT COMMIT is measured that way, on the same box — a package
without the `kalman` keyword runs the first two variants only.  Inputs: oracle/tracker_ref.synth_sequence (8 scenes dealt to the streams).
"""
import argparse
import ctypes
import inspect
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = 8


def pct(v):
    return "p50 %9.1f  p10 %9.1f  p90 %9.1f us" % (np.percentile(v, 50), np.percentile(v, 10), np.percentile(v, 90))


def variants(cl):
    out = {"use_kalman=False": dict(use_kalman=False), "kalman=host": dict(use_kalman=True)}
    if "kalman" in inspect.signature(cl.Tracker.__init__).parameters:
        out["kalman=host"]["kalman"] = "host"
        out["kalman=device"] = dict(use_kalman=True, kalman="device")
    return out


def frames_for(S, frames, dev, tracker_ref, k=300, objects=68):
    scenes = [tracker_ref.synth_sequence(s, frames=frames + 3 * (SCENES - 1), objects=objects + s % 3, k=k) for s in range(min(S, SCENES))]
    pick = lambda s, f: scenes[s % len(scenes)][f + 3 * ((s // len(scenes)) % SCENES)]
    return [[torch.from_numpy(np.stack([pick(s, f)[j] for s in range(S)])).to(dev) for j in range(4)] for f in range(frames)]


def steps_of(make, step, data, warmup):
    """`make(kw)` builds one tracker per variant; `step(tracker, frame)` advances it.  Alternates the variants frame by frame."""
    trackers = {name: make(kw) for name, kw in VARIANTS.items()}
    times = {name: [] for name in trackers}
    torch.cuda.synchronize()
    for f, fr in enumerate(data):
        for name, t in trackers.items():
            t0 = time.perf_counter()
            step(t, fr)
            torch.cuda.synchronize()
            if f >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e6)
    return trackers, times


def report(title, times, rows):
    print(title)
    for name, v in times.items():
        print(f"  {name:18s} {pct(v)}")
    base = np.median(times["use_kalman=False"])
    for name, v in times.items():
        if name != "use_kalman=False":
            print(f"  {name:18s} - use_kalman=False = {np.median(v) - base:9.1f} us per step ({rows} rows)")
    sys.stdout.flush()


def kernel_alone(R, dev, reps, _lib, _Mapped):
    lib = _lib.load()
    rng = np.random.default_rng(R)
    c, s = rng.uniform(0, 0.7, (R, 2)), rng.uniform(0.03, 0.3, (R, 2))
    det = torch.from_numpy(np.concatenate([c, c + s], 1).astype(np.float32)).to(dev)
    tabs = [(torch.empty((R, 8), device=dev, dtype=torch.float64), torch.empty((R, 64), device=dev, dtype=torch.float64)) for _ in range(2)]
    box = torch.empty((R, 4), device=dev, dtype=torch.float32)
    rows = np.arange(R, dtype=np.int32)
    lists = _Mapped(12 * R)
    li = lists.np.view(np.int32).reshape(3, R)
    li[0], li[1], li[2] = -1, rows, 1
    out = _Mapped(36 * R)
    cur = torch.cuda.current_stream(dev)
    stream = ctypes.c_void_p(cur.cuda_stream)

    def call(i, old=True):
        (ox, oP), (nx, nP) = tabs[i & 1], tabs[~i & 1]
        _lib.check(lib.cnl_track_kalman_f64(ox.data_ptr() if old else None, oP.data_ptr() if old else None, det.data_ptr(), lists.ptr, lists.ptr + 4 * R,
                                            lists.ptr + 8 * R, R, nx.data_ptr(), nP.data_ptr(), box.data_ptr(), out.ptr, out.ptr + 32 * R, stream),
                   "cnl_track_kalman_f64")
    call(0, old=False)                              # births
    cur.synchronize()
    li[0] = rows                                    # from here on: every row matched with its detection and predicted
    for i in range(1, 6):
        call(i)
    cur.synchronize()
    t_ev, t_wall = [], []
    for i in range(6, 6 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(i); e1.record(); cur.synchronize()
        t_ev.append(e0.elapsed_time(e1) * 1e3)
    for i in range(6 + reps, 6 + 2 * reps):
        t0 = time.perf_counter()
        call(i)
        cur.synchronize()
        t_wall.append((time.perf_counter() - t0) * 1e6)
    skipped = int(np.count_nonzero(out.np[32 * R:36 * R].view(np.int32)))
    print(f"  R = {R:5d} rows   HIP events {pct(t_ev)}   launch + synchronise {pct(t_wall)}   skipped rows {skipped}")
    sys.stdout.flush()


def main():
    global VARIANTS
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", default="70,2240,4480")
    ap.add_argument("--package", default=os.path.join(ROOT, "centernet-lightning_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import centernet_lightning_amd as cl
    from centernet_lightning_amd import _lib
    from centernet_lightning_amd.tracker import _Mapped
    import tracker_ref                              # input recipe only
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    VARIANTS = variants(cl)
    print(f"kalman_bench: {torch.cuda.get_device_name(0)}, package {os.path.relpath(os.path.dirname(cl.__file__), ROOT)}, {a.steps} steps after {a.warmup} "
          "warm-up steps, wall time per step incl. the closing synchronisation")
    S, frames = a.streams, a.steps + a.warmup
    data = frames_for(S, frames, dev, tracker_ref)
    banks, times = steps_of(lambda kw: cl.TrackerBank(num_streams=S, device=dev, **kw), lambda b, fr: b.update_batch(*fr), data, a.warmup)
    rows = {name: int(b._off[S]) for name, b in banks.items()}
    report(f"TrackerBank.update_batch, S = {S}, k = 300, pooled rows at the end {sorted(set(rows.values()))}", times, max(rows.values()))
    _, times1 = steps_of(lambda kw: cl.Tracker(device=dev, **kw), lambda t, fr: t.update(fr[0][0], fr[1][0], fr[2][0], fr[3][0]), data, a.warmup)
    report("Tracker.update, one stream, k = 300", times1, rows[next(iter(rows))] // S)
    if "kalman=device" in VARIANTS:
        print("cnl_track_kalman_f64 alone (every row matched and predicted)")
        for R in (int(x) for x in a.rows.split(",")):
            kernel_alone(R, dev, a.steps, _lib, _Mapped)


if __name__ == "__main__":
    main()
