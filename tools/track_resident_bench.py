"""TrackerBank with the track life cycle on the device (lifecycle="device") beside the bank of today (lifecycle="host"), in one process.

    python tools/track_resident_bench.py [--cases readme:32,readme:64,small:32] [--variants plain,byte,kalman] [--steps 150] [--warmup 30]
                                         [--lifecycles host,device] [--max-tracks 256] [--package-root DIR]

The scenes are those of tools/track_streams_bench.py (readme: k = 300 detections, ~58 kept, ~70 tracks per stream; small: k = 48, 12 objects;
oracle/tracker_ref.synth_sequence, 8 scenes dealt to the streams with different time offsets).  Per case, S and variant (plain; byte:
low_threshold = 0.1; kalman: use_kalman, kalman = "device") the banks are stepped on the same [S, k, ...] device tensors, alternating:
  enqueue   host time of `update_batch` alone (the call returns; for lifecycle="host" that includes its synchronisations), step by step
            alternating between the banks, each step then closed by a device synchronisation that is not counted;
  run       wall time per step of a run of `--run` steps closed by ONE final synchronisation, runs alternating between the banks.
`--lifecycles host --package-root DIR` measures the host mode of another checkout (the parent commit) with this same script: its package is
imported from DIR and no `lifecycle` keyword is passed.
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"readme": dict(k=300, objects=68), "small": dict(k=48, objects=12)}
VARIANTS = {"plain": {}, "byte": dict(low_threshold=0.1), "kalman": dict(use_kalman=True, kalman="device")}
SCENES = 8


def pct(v):
    return "p50 %8.1f  p10 %8.1f  p90 %8.1f us" % (np.percentile(v, 50), np.percentile(v, 10), np.percentile(v, 90))


def ids_of(bank, S):
    return [[t.track_id for t in bank[s].tracks] for s in range(S)]


def run(cl, scenes, case, S, variant, a, dev):
    kw = CASES[case]
    frames = a.warmup + a.steps + a.runs * a.run
    pick = lambda s, f: scenes[s % len(scenes)][f + 3 * ((s // len(scenes)) % SCENES)]
    data = [[torch.from_numpy(np.stack([pick(s, f)[j] for s in range(S)])).to(dev) for j in range(4)] for f in range(frames)]
    banks = {}
    for lc in a.lifecycles:
        extra = {} if lc == "host" else dict(lifecycle="device", max_tracks=a.max_tracks)
        banks[lc] = cl.TrackerBank(num_streams=S, device=dev, **VARIANTS[variant], **extra)
    torch.cuda.synchronize()
    enq = {lc: [] for lc in banks}
    f = 0
    for f in range(a.warmup + a.steps):
        for lc, bank in banks.items():
            t0 = time.perf_counter()
            bank.update_batch(*data[f])
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if f >= a.warmup:
                enq[lc].append((t1 - t0) * 1e6)
    wall = {lc: [] for lc in banks}
    f += 1
    for _ in range(a.runs):
        for lc, bank in banks.items():
            t0 = time.perf_counter()
            for g in range(f, f + a.run):
                bank.update_batch(*data[g])
            torch.cuda.synchronize()
            wall[lc].append((time.perf_counter() - t0) * 1e6 / a.run)
        f += a.run
    rows = np.mean([len(ids) for ids in ids_of(banks[a.lifecycles[0]], S)])
    print(f"case {case} (k = {kw['k']})  S = {S:3d}  variant {variant:6s}  steps = {a.steps}, {a.runs} runs of {a.run} steps;  mean rows per stream at the end {rows:.1f}")
    for lc in banks:
        print(f"  lifecycle={lc:6s}  enqueue per step {pct(enq[lc])}   run: wall per step {pct(wall[lc])}")
    if len(banks) == 2:
        print(f"  host p50 / device p50: enqueue x{np.percentile(enq['host'], 50) / np.percentile(enq['device'], 50):.2f}, "
              f"run x{np.percentile(wall['host'], 50) / np.percentile(wall['device'], 50):.2f};  same track ids in every stream: "
              f"{ids_of(banks['host'], S) == ids_of(banks['device'], S)}")
        banks["device"].check()
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="readme:32,readme:64,small:32")
    ap.add_argument("--variants", default="plain,byte,kalman")
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--run", type=int, default=20)
    ap.add_argument("--lifecycles", default="host,device")
    ap.add_argument("--max-tracks", type=int, default=256)
    ap.add_argument("--package-root", default=ROOT)
    a = ap.parse_args()
    a.lifecycles = a.lifecycles.split(",")
    sys.path.insert(0, os.path.join(a.package_root, "centernet-lightning_amd"))
    sys.path.insert(0, os.path.join(a.package_root, "oracle"))
    import centernet_lightning_amd as cl
    import tracker_ref                            # (input recipe only)
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    print(f"track_resident_bench: {torch.cuda.get_device_name(0)}, package {os.path.relpath(os.path.dirname(cl.__file__), ROOT)}, lifecycles {a.lifecycles}, "
          f"max_tracks = {a.max_tracks}")
    scenes = {}
    for item in a.cases.split(","):
        case, S = item.split(":")
        S = int(S)
        frames = a.warmup + a.steps + a.runs * a.run
        if case not in scenes:
            kw = CASES[case]
            scenes[case] = [tracker_ref.synth_sequence(s, frames=frames + 3 * (SCENES - 1), objects=kw["objects"] + s % 3, k=kw["k"]) for s in range(SCENES)]
        for variant in a.variants.split(","):
            run(cl, scenes[case], case, S, variant, a, dev)


if __name__ == "__main__":
    main()
