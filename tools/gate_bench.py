"""Class / motion gate measurement: what class_aware and motion_gate cost a tracking step, against the ungated step on the same box.

    python tools/gate_bench.py [--streams 32] [--steps 40] [--warmup 10] [--rounds 3]

In ONE process, `--rounds` times over: step by step alternating between the variants on the same frames, each step closed by a device
synchronisation, median (p10, p90) of the wall time per step over `--steps` steps after `--warmup`:
  (a) TrackerBank.update_batch at S streams, k = 300 detections per stream (the scenes of tools/byte_bench.py: ~58 kept detections and ~70 tracks
      per stream), use_kalman=True, kalman="device" throughout (the motion gate needs it): ungated, class_aware, motion_gate, both;
  (b) Tracker.update at one stream, the same four variants;
  (c) the launches alone, by HIP events, on the ungated bank's final tables and the last frame, records in mapped host memory as in the product:
      the frame entry (ONE launch: the cost kernel) of stream 0 — cnl_track_frame_low_f32 against cnl_track_frame_gated_f32 with each gate —
      and the streams entry (cost launch + assign launch) of all S streams — cnl_track_streams_low_f32 against cnl_track_streams_gated_f32 —
      and, to tell the two launches of that entry apart, the batched solver alone (cnl_lsap_batch_f64: stage 1 of the assign launch) on the
      re-ID matrices that each variant's cost launch left in the workspace.
With the options off there is nothing to compare: those trackers call the entry points they called before.
The scenes carry one class; the labels here are the sign of the first embedding element (stable per object: the identity embedding dominates its
noise), so about half of the pairs are cross-class.  The trackers of one variant group therefore do not all hold the same tracks: a gate changes
the matches.  The rows at the end are printed per variant.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from byte_bench import frames_for, pct          # noqa: E402  (the scenes and the percentile line of the BYTE bench)

KAL = dict(use_kalman=True, kalman="device")
VARIANTS = {"ungated": dict(), "class_aware": dict(class_aware=True), "motion_gate": dict(motion_gate=True),
            "class + motion": dict(class_aware=True, motion_gate=True)}


def alternate(make, step, data, warmup):
    trackers = {name: make(dict(KAL, **kw)) for name, kw in VARIANTS.items()}
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
    base = np.median(times["ungated"])
    for name, v in times.items():
        delta = "" if name == "ungated" else f"   - ungated = {np.median(v) - base:+8.1f} us ({100 * (np.median(v) / base - 1):+.1f} %)"
        print(f"  {name:16s} {pct(v)}{delta}")
    sys.stdout.flush()


def events(call, cur, reps):
    for _ in range(5):
        call()
    cur.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); cur.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return t


def launches_alone(bank, frame, reps, _lib, th):
    lib = _lib.load()
    dev, S = bank.device, bank.num_streams
    d_box, d_label, d_score, d_emb = (frame[j].contiguous() for j in range(4))
    k, E = int(d_emb.shape[1]), int(d_emb.shape[2])
    off, table = bank._off, bank._table
    R, T_max = int(off[S]), max(int(off[s + 1] - off[s]) for s in range(S))
    cur = torch.cuda.current_stream(dev)
    stream = ctypes.c_void_p(cur.cuda_stream)
    labels = th._Mapped(4 * max(R, 1))
    labels.np.view(np.int32)[:R] = [int(t.label) for s in range(S) for t in bank[s].tracks]
    det, low, box_thr = float(bank.detection_threshold), 0.1, float(bank.box_threshold)

    def gate(cls, motion):
        g = _lib.TrackGate(None, None, None, 0.0, 1.0)
        if cls:
            g.trk_label = labels.ptr
        if motion:
            g.kx, g.kP, g.motion_gate = table.kx.data_ptr(), table.kP.data_ptr(), th.CHI2INV95_4
        return g
    gates = {"class_aware": gate(1, 0), "motion_gate": gate(0, 1), "class + motion": gate(1, 1)}

    # ---- the frame entry: ONE launch, stream 0's rows
    T0 = int(off[1] - off[0])
    rec = th._Mapped(th.frame_low_layout(k, T0, True).bytes)
    args = (d_emb[0].data_ptr(), d_box[0].data_ptr(), d_score[0].data_ptr(), d_label[0].data_ptr(), 1, k, E, det, low, table.emb.data_ptr(), table.box.data_ptr(),
            T0, 1, 0, 1, rec.ptr, rec.nbytes)
    rows = {"ungated": events(lambda: _lib.check(lib.cnl_track_frame_low_f32(*args, stream)), cur, reps)}
    for name, g in gates.items():
        rows[name] = events(lambda g=g: _lib.check(lib.cnl_track_frame_gated_f32(*args, ctypes.byref(g), stream)), cur, reps)
        n = int(rec.np[:4].view(np.int32)[0])
        reid = rec.np[rec.np[24:28].view(np.int32)[0]:][:8 * n * T0].view(np.float64)
        rows[name + " gated share"] = float((reid == th.GATE_COST).mean())
    print(f"the cost launch alone (frame entry, k = {k}, T = {T0}, low-score stage on), HIP events")
    _rows(rows)

    # ---- the streams entry: cost launch + assign launch, all streams
    stride = th.streams_low_layout(k, T_max, True).bytes
    ws = torch.empty(th.streams_low_workspace_bytes(S, k, R), device=dev, dtype=torch.uint8)
    recs = th._Mapped(S * stride)
    ctl = th._Mapped(4 * (2 * S + 1))
    ctl.np.view(np.int32)[:S] = np.arange(S)
    ctl.np.view(np.int32)[S:2 * S + 1] = off
    args = (d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr(), 1, S, S, ctl.ptr, k, E, det, float(bank.reid_threshold), box_thr, low,
            box_thr, table.emb.data_ptr(), table.box.data_ptr(), ctl.ptr + 4 * S, None, R, T_max, 1, 0, 1, ws.data_ptr(), ws.numel(), recs.ptr, stride)
    # ... and, behind each variant, stage 1 of the assign launch ALONE: the batched solver (cnl_lsap_batch_f64, the device code the assign kernel
    # calls) on the S re-ID matrices that variant's cost launch left in the workspace
    n_rows = torch.zeros(S, dtype=torch.int32, device=dev)
    n_cols = torch.from_numpy(np.diff(off).astype(np.int32)).to(dev)
    cost_off = torch.from_numpy((k * off[:S]).astype(np.int64)).to(dev)
    col_off = torch.arange(S, dtype=torch.int64, device=dev) * k
    col4row = torch.empty(S * k, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)

    def solver():
        n_rows.copy_(torch.from_numpy(np.array([recs.np[s * stride:s * stride + 4].view(np.int32)[0] for s in range(S)], np.int32)))
        cur.synchronize()
        call = lambda: _lib.check(lib.cnl_lsap_batch_f64(ws.data_ptr(), cost_off.data_ptr(), n_cols.data_ptr(), n_rows.data_ptr(), n_cols.data_ptr(), S, k, T_max,
                                                         col4row.data_ptr(), col_off.data_ptr(), status.data_ptr(), stream))
        t = events(call, cur, reps)
        assert not status.any().item()
        return t
    rows = {"ungated": events(lambda: _lib.check(lib.cnl_track_streams_low_f32(*args, stream)), cur, reps)}
    solve = {"ungated": solver()}
    for name, g in gates.items():
        rows[name] = events(lambda g=g: _lib.check(lib.cnl_track_streams_gated_f32(*args, ctypes.byref(g), stream)), cur, reps)
        rows[name + " status != 0"] = sum(int(recs.np[s * stride + 12:s * stride + 16].view(np.int32)[0] != 0) for s in range(S))
        solve[name] = solver()
    print(f"the association pass alone (streams entry: cost launch + assign launch, S = {S}, R = {R} rows, T_max = {T_max}), HIP events")
    _rows(rows)
    print(f"stage 1 of the assign launch alone (cnl_lsap_batch_f64 on the {S} re-ID matrices each variant's cost launch wrote), HIP events")
    _rows(solve)


def _rows(rows):
    base = np.median(rows["ungated"])
    for name, v in rows.items():
        if isinstance(v, list):
            delta = "" if name == "ungated" else f"   - ungated = {np.median(v) - base:+8.1f} us ({100 * (np.median(v) / base - 1):+.1f} %)"
            print(f"  {name:16s} {pct(v)}{delta}")
        else:
            print(f"  {name:28s} {v:.3g}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import centernet_lightning_amd as cl
    from centernet_lightning_amd import _lib
    from centernet_lightning_amd import _track_host as th
    import tracker_ref                              # input recipe only
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    print(f"gate_bench: {torch.cuda.get_device_name(0)}, {a.rounds} rounds of {a.steps} steps after {a.warmup} warm-up steps, wall time per step incl. the "
          "closing synchronisation; use_kalman=True, kalman='device' in every variant")
    S, frames = a.streams, a.steps + a.warmup
    data = frames_for(S, frames, dev, tracker_ref)
    for fr in data:
        fr[1] = (fr[3][..., 0] > 0).to(torch.int64)      # two classes, stable per object
    for r in range(a.rounds):
        print(f"== round {r + 1}")
        banks, times = alternate(lambda kw: cl.TrackerBank(num_streams=S, device=dev, **kw), lambda b, fr: b.update_batch(*fr), data, a.warmup)
        report(f"TrackerBank.update_batch, S = {S}, k = 300, pooled rows at the end { {n: int(b._off[S]) for n, b in banks.items()} }", times)
        singles, times1 = alternate(lambda kw: cl.Tracker(device=dev, **kw), lambda t, fr: t.update(fr[0][0], fr[1][0], fr[2][0], fr[3][0]), data, a.warmup)
        report(f"Tracker.update, one stream, k = 300, tracks at the end { {n: len(t.tracks) for n, t in singles.items()} }", times1)
        launches_alone(banks["ungated"], data[-1], a.steps, _lib, th)


if __name__ == "__main__":
    main()
