"""BYTE low-score association measurement: what low_threshold costs a tracking step, and that the path without it kept its time.

    python tools/byte_bench.py [--streams 32] [--steps 40] [--warmup 10] [--low 0.1] [--package DIR [--label TEXT]]
    python tools/byte_bench.py --rounds 5 --parent-package DIR --parent-lib FILE --parent-label COMMIT       (the same-box comparison)

In ONE process, step by step alternating between the variants on the same frames, each step closed by a device synchronisation, median
(p10, p90) of the wall time per step over `--steps` steps after `--warmup`:
  (a) TrackerBank.update_batch at S streams, k = 300 detections per stream (~58 kept, ~70 tracks per stream: the shapes of
      profiles/track_streams_bench.txt), with low_threshold=None and low_threshold=`--low`;
  (b) Tracker.update at one stream, the same two variants;
  (c) the association pass alone (cnl_track_streams_f32 / cnl_track_streams_low_f32 on the bank's final table and the last frame, records in
      mapped host memory as in the product), by HIP events.
`--package DIR` imports centernet_lightning_amd from DIR (a checkout of another commit's centernet-lightning_amd/, with CENTERNET_GFX950_LIB
naming a built library) instead of this tree, printed as `--label`; a package without the `low_threshold` keyword runs the None rows only.
`--rounds N --parent-package DIR --parent-lib FILE --parent-label COMMIT` does the same-box comparison of the None rows itself: N rounds, in
each a fresh child process of this tool for the parent commit's package and library (a checkout of that commit, built) and then one for
this tree, and at the end the p50s of the None rows of both, round by round: they are the same entry points, so the two ranges should
overlap.  Inputs: oracle/tracker_ref.synth_sequence (8 scenes dealt to the streams); its clutter puts ~150
of the 300 detections between 0.1 and 0.3, so the low stage is a large one.
"""
import argparse
import ctypes
import inspect
import os
import re
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = 8


def pct(v):
    return "p50 %9.1f  p10 %9.1f  p90 %9.1f us" % (np.percentile(v, 50), np.percentile(v, 10), np.percentile(v, 90))


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


def report(title, times):
    print(title)
    for name, v in times.items():
        print(f"  {name:20s} {pct(v)}")
    base = np.median(times["low_threshold=None"])
    for name, v in times.items():
        if name != "low_threshold=None":
            print(f"  {name:20s} - low_threshold=None = {np.median(v) - base:9.1f} us per step")
    sys.stdout.flush()


def association_alone(bank, frame, low, reps, _lib, th):
    """The association pass on `bank`'s table and `frame`, by HIP events: the entry without (low None) or with the low stage."""
    lib = _lib.load()
    dev = bank.device
    S = bank.num_streams
    d_box, d_score, d_emb = (frame[j].contiguous() for j in (0, 2, 3))
    k, E = int(d_emb.shape[1]), int(d_emb.shape[2])
    off = bank._off
    R, T_max = int(off[S]), max(int(off[s + 1] - off[s]) for s in range(S))
    on = low is not None
    stride = (th.streams_low_layout if on else th.streams_layout)(k, T_max, True).bytes
    ws = torch.empty((th.streams_low_workspace_bytes if on else th.streams_workspace_bytes)(S, k, R), device=dev, dtype=torch.uint8)
    rec = th._Mapped(S * stride)
    ctl = th._Mapped(4 * (2 * S + 1))
    ctl.np.view(np.int32)[:S] = np.arange(S)
    ctl.np.view(np.int32)[S:2 * S + 1] = off
    elig = th._Mapped(max(R, 1))
    elig.np[:R] = [t.state is th.TrackState.ACTIVE for s in range(S) for t in bank[s].tracks]
    cur = torch.cuda.current_stream(dev)
    head = (d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), None, 0, S, S, ctl.ptr, k, E, float(bank.detection_threshold), float(bank.reid_threshold),
            float(bank.box_threshold))
    tables = (bank._emb.data_ptr(), bank._box.data_ptr(), ctl.ptr + 4 * S)
    tail = (R, T_max, 1, 0, 1, ws.data_ptr(), ws.numel(), rec.ptr, stride, ctypes.c_void_p(cur.cuda_stream))

    def call():
        if on:
            _lib.check(lib.cnl_track_streams_low_f32(*head, float(low), float(bank.box_threshold), *tables, elig.ptr, *tail), "cnl_track_streams_low_f32")
        else:
            _lib.check(lib.cnl_track_streams_f32(*head, *tables, *tail), "cnl_track_streams_f32")
    for _ in range(5):
        call()
    cur.synchronize()
    t_ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); cur.synchronize()
        t_ev.append(e0.elapsed_time(e1) * 1e3)
    hdr = [rec.np[s * stride:s * stride + (96 if on else 64)].view(np.int32) for s in range(S)]
    extra = f"   low detections per stream {np.mean([h[16] for h in hdr]):.0f}, low matches {np.mean([h[17] for h in hdr]):.1f}" if on else ""
    print(f"  low_threshold={low!s:5s} R = {R} rows, T_max = {T_max}   HIP events {pct(t_ev)}   status != 0: {sum(int(h[3] != 0) for h in hdr)}{extra}")
    sys.stdout.flush()


def rounds(a):
    """The same-box comparison: children of this tool, parent commit and this tree in turn, and the None rows' p50s side by side."""
    me = [sys.executable, os.path.abspath(__file__), "--streams", str(a.streams), "--steps", str(a.steps), "--warmup", str(a.warmup), "--low", str(a.low)]
    sides = {f"parent commit {a.parent_label}": (me + ["--package", a.parent_package, "--label", f"parent commit {a.parent_label}"],
                                                 dict(os.environ, CENTERNET_GFX950_LIB=os.path.abspath(a.parent_lib))),
             "this tree": (me + ["--label", "this tree"], dict(os.environ))}
    p50 = {side: {"bank": [], "tracker": []} for side in sides}
    for r in range(a.rounds):
        for side, (cmd, env) in sides.items():
            print(f"== round {r + 1}: {side}")
            sys.stdout.flush()
            out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True).stdout
            print(out, end="")
            rows = re.findall(r"low_threshold=None\s+p50\s+([0-9.]+)", out)
            p50[side]["bank"].append(float(rows[0]))
            p50[side]["tracker"].append(float(rows[1]))
    print("== low_threshold=None, p50 per round (us)")
    for what, title in (("bank", f"TrackerBank.update_batch, S = {a.streams}"), ("tracker", "Tracker.update, one stream")):
        for side, v in p50.items():
            print(f"  {title:36s} {side:28s} " + " ".join(f"{x:8.1f}" for x in v[what]) + f"   range {min(v[what]):.1f} .. {max(v[what]):.1f}")
    sys.stdout.flush()


def main():
    global VARIANTS
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--low", type=float, default=0.1)
    ap.add_argument("--package", default=os.path.join(ROOT, "centernet-lightning_amd"))
    ap.add_argument("--label", default=None)
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--parent-package", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-label", default="")
    a = ap.parse_args()
    if a.rounds:
        if not (a.parent_package and a.parent_lib):
            ap.error("--rounds needs --parent-package and --parent-lib")
        return rounds(a)
    sys.path.insert(0, a.package)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import centernet_lightning_amd as cl
    from centernet_lightning_amd import _lib
    from centernet_lightning_amd import _track_host as th
    import tracker_ref                              # input recipe only
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    VARIANTS = {"low_threshold=None": dict()}
    has_low = "low_threshold" in inspect.signature(cl.Tracker.__init__).parameters
    if has_low:
        VARIANTS[f"low_threshold={a.low}"] = dict(low_threshold=a.low)
    print(f"byte_bench: {torch.cuda.get_device_name(0)}, {a.label or 'package ' + os.path.relpath(os.path.dirname(cl.__file__), ROOT)}, {a.steps} steps after {a.warmup} "
          "warm-up steps, wall time per step incl. the closing synchronisation")
    S, frames = a.streams, a.steps + a.warmup
    data = frames_for(S, frames, dev, tracker_ref)
    banks, times = steps_of(lambda kw: cl.TrackerBank(num_streams=S, device=dev, **kw), lambda b, fr: b.update_batch(*fr), data, a.warmup)
    rows = {name: int(b._off[S]) for name, b in banks.items()}
    report(f"TrackerBank.update_batch, S = {S}, k = 300, pooled rows at the end {rows}", times)
    if has_low:
        lows = [len(x) for x in banks[f"low_threshold={a.low}"].last_low_matches]
        print(f"  low matches in the last step: {sum(lows)} over {S} streams; bytes over PCIe in the last step: "
              + ", ".join(f"{name} {b.d2h_bytes}" for name, b in banks.items()))
    _, times1 = steps_of(lambda kw: cl.Tracker(device=dev, **kw), lambda t, fr: t.update(fr[0][0], fr[1][0], fr[2][0], fr[3][0]), data, a.warmup)
    report("Tracker.update, one stream, k = 300", times1)
    if has_low:
        print("association pass alone (both launches), on the low_threshold=None bank's final table and the last frame")
        for low in (None, a.low):
            association_alone(banks["low_threshold=None"], data[-1], low, a.steps, _lib, th)


if __name__ == "__main__":
    main()
