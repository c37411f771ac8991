"""The zone counter measured: its launch, the call, what it adds to a run of device-life-cycle steps, and the host loop it replaces.

    python tools/zones_bench.py [--streams 32] [--reps 20] [--steps 20] [--warmup 10] [--out profiles/zones_bench.txt]

S streams, max_tracks = 256, the scenes of tools/byte_bench.py (k = 300 detections, about 78 reported tracks per stream), 4 zones and 2 lines
in normalised coordinates.  Median (p10, p90) of `--reps`:
  (a) cnl_track_zones_f64 alone, by HIP events, on the outputs of one bank step (the state keeps alternating between its banks);
  (b) ZoneCounter.update as a call: wall time from the call to the end of a closing synchronisation;
  (c) a run of `--steps` TrackerBank(lifecycle="device").update_batch steps closed by ONE synchronisation, with ZoneCounter.update behind
      every step and without it — the bank alone is the parent commit's behaviour: this feature changes no line of it.  The two kinds of run
      alternate on the same detections;
  (d) the path the counter replaces: download the step's four output tensors and run tests/zones_ref.py (the numpy restatement, a Python loop
      over the tracks) on the host — per step, and checked to give the counter's events.
"""
import argparse
import ctypes
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from byte_bench import frames_for, pct          # noqa: E402  (the scenes and the percentile line of the BYTE bench)

M = 256
LINES = []


def say(line=""):
    print(line)
    sys.stdout.flush()
    LINES.append(line)


def geometry(cl):
    zones = [cl.Zone([(0.05, 0.55), (0.95, 0.55), (0.95, 0.95), (0.05, 0.95)], dwell_alert=25),
             cl.Zone([(0.1, 0.1), (0.45, 0.1), (0.45, 0.45), (0.3, 0.3), (0.1, 0.45)]),
             cl.Zone([(0.5 + 0.2 * np.cos(k * np.pi / 8), 0.5 + 0.2 * np.sin(k * np.pi / 8)) for k in range(16)], dwell_alert=10),
             cl.Zone([(0.6, 0.05), (0.95, 0.05), (0.95, 0.4)], labels=[0])]
    lines = [cl.Line(0.0, 0.5, 1.0, 0.5), cl.Line(0.5, 1.0, 0.5, 0.0)]
    return dict(zones=zones, lines=lines, max_tracks=M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zones_bench.txt"))
    a = ap.parse_args()
    import centernet_lightning_amd as cl
    from centernet_lightning_amd import _lib
    import tracker_ref                              # input recipe only
    import zones_ref
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "zones_bench measures on a HIP device"
    dev = torch.device("cuda:0")
    S = a.streams
    say(f"command: python tools/zones_bench.py --streams {S} --reps {a.reps} --steps {a.steps} --warmup {a.warmup}")
    say(f"{torch.cuda.get_device_name(0)}; S = {S} streams, max_tracks = {M}, k = 300 detections, 4 zones (4, 5, 16, 3 vertices), 2 lines; "
        f"median (p10, p90) of {a.reps}")
    frames = a.warmup + a.steps
    data = frames_for(S, frames, dev, tracker_ref)
    bank_kw = dict(num_streams=S, device=dev, lifecycle="device", max_tracks=M)
    geo = geometry(cl)

    # the bank's outputs of every step, once: the inputs of (a), (b) and (d)
    bank = cl.TrackerBank(**bank_kw)
    tracks = [bank.update_batch(*fr) for fr in data]
    torch.cuda.synchronize()
    counts = torch.stack([t["count"] for t in tracks[a.warmup:]]).float()
    say(f"reported tracks per stream over the measured steps: mean {float(counts.mean()):.1f}, max {int(counts.max())}")

    # (a) the launch alone
    zc = cl.ZoneCounter(S, device=dev, **geo)
    for t in tracks[:a.warmup]:
        out = zc.update(t)
    lib = _lib.load()
    t = tracks[a.warmup]
    lv = zc._live_list(tuple(range(S)))
    args = [_lib.TrackZones(t["bboxes"].data_ptr(), t["track_ids"].data_ptr(), t["labels"].data_ptr(), t["count"].data_ptr(), lv.data_ptr(),
                            zc._geometry_dev.data_ptr(), zc._state.data_ptr(), zc._status.data_ptr(),
                            *(out[k].data_ptr() for k in ("inside", "dwell", "occupancy", "zone_counts", "line_counts", "events", "event_count")),
                            S, S, M, M, zc.Z, zc.Ln, zc.max_events, zc.max_absent, 0, int(t["bboxes"].dtype == torch.float64), b, 0) for b in (0, 1)]
    stream = _lib.stream(dev)
    flip = [zc._bank]
    times = []
    torch.cuda.synchronize()
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.cnl_track_zones_f64(ctypes.byref(args[flip[0]]), stream), "cnl_track_zones_f64")
        e1.record()
        torch.cuda.synchronize()
        flip[0] ^= 1
        times.append(e0.elapsed_time(e1) * 1e3)
    say(f"(a) cnl_track_zones_f64 alone, HIP events, {S} workgroups of 256 threads                    {pct(times)}")

    # (b) the call
    zc = cl.ZoneCounter(S, device=dev, **geo)
    for t in tracks[:a.warmup]:
        zc.update(t)
    torch.cuda.synchronize()
    times = []
    for i in range(a.reps):
        t = tracks[a.warmup + i % a.steps]
        t0 = time.perf_counter()
        zc.update(t)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    say(f"(b) ZoneCounter.update: call + closing synchronisation                                      {pct(times)}")

    # (c) runs of steps closed by one synchronisation
    runs = {"bank alone": [], "bank + counter": []}
    for rep in range(a.reps + 2):
        for name in runs:
            bank = cl.TrackerBank(**bank_kw)
            zc = cl.ZoneCounter(S, device=dev, **geo) if name == "bank + counter" else None
            for fr in data[:a.warmup]:
                out = bank.update_batch(*fr)
                if zc is not None:
                    zc.update(out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for fr in data[a.warmup:]:
                out = bank.update_batch(*fr)
                if zc is not None:
                    zc.update(out)
            torch.cuda.synchronize()
            if rep >= 2:
                runs[name].append((time.perf_counter() - t0) * 1e6)
    say(f"(c) {a.steps} steps of TrackerBank(lifecycle='device').update_batch, S = {S}, k = 300, closed by ONE synchronisation (the runs alternate)")
    for name, v in runs.items():
        say(f"  {name:16s} {pct(v)}   per step {np.median(v) / a.steps:8.1f} us")
    diff = np.asarray(runs["bank + counter"]) - np.asarray(runs["bank alone"])
    say(f"  per-run differences, with - without: median {np.median(diff):+.1f} us (p10 {np.percentile(diff, 10):+.1f}, p90 {np.percentile(diff, 90):+.1f}), "
        f"{np.median(diff) / a.steps:+.1f} us per step")

    # (d) the host path: download, then the numpy restatement
    zc = cl.ZoneCounter(S, device=dev, **geo)
    ref = zones_ref.ZoneCounterRef(S, **geo)
    down, loop, equal = [], [], True
    for i, t in enumerate(tracks):
        got = zc.update(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = {k: v.cpu().numpy() for k, v in t.items()}
        t1 = time.perf_counter()
        want = ref.update(host)
        t2 = time.perf_counter()
        if i >= a.warmup:
            down.append((t1 - t0) * 1e6)
            loop.append((t2 - t1) * 1e6)
        equal = equal and all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in want)
    say(f"(d) the host path per step: download of bboxes, track_ids, labels, count ({sum(v.numel() * v.element_size() for v in tracks[0].values())} bytes)   {pct(down)}")
    say(f"    tests/zones_ref.py on the downloaded arrays (numpy predicates, a Python loop over the tracks)    {pct(loop)}")
    say(f"    the counter's outputs equal the restatement's on every one of the {len(tracks)} steps: {equal}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
