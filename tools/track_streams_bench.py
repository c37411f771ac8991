"""Many-streams tracker measurement: one TrackerBank step for S streams beside a loop over S independent Tracker objects.

    python tools/track_streams_bench.py [--streams 1,8,32,64] [--steps 200] [--warmup 30] [--cases readme,small] [--bank-only]

Per case (readme: k = 300 detections, ~58 kept, ~70 tracks per stream; small: k = 48, 12 objects) and per S, in ONE process, step by
step alternating (i) `bank.update_batch` on the [S, k, ...] device tensors and (ii) `for s: trackers[s].update(...)` on the same
frames, each closed by a device synchronisation: p50 / p10 / p90 of the wall time per step, d2h_bytes of both, the association pass
alone (cnl_track_streams_f32 + the synchronisation on a frozen state), and the assignment kernel alone (cnl_lsap_batch_f64, the S
re-ID matrices of one step in one launch) against scipy alone on the same matrices.  Inputs: oracle/tracker_ref.synth_sequence (8
distinct scenes, dealt to the streams with different time offsets).  `--bank-only` runs only (i) (for a HIP-trace of the bank's calls).
"""
import argparse
import ctypes
import os
import sys
import time
import warnings

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import centernet_lightning_amd as cl          # noqa: E402
from centernet_lightning_amd import _lib      # noqa: E402
from centernet_lightning_amd.tracker import _Mapped      # noqa: E402
import tracker_ref                            # noqa: E402  (input recipe only)

CASES = {"readme": dict(k=300, objects=68), "small": dict(k=48, objects=12)}
SCENES = 8


def pct(v):
    return "p50 %8.1f  p10 %8.1f  p90 %8.1f us" % (np.percentile(v, 50), np.percentile(v, 10), np.percentile(v, 90))


def lsap_alone(mats, dev, reps=50):
    lib = _lib.load()
    B = len(mats)
    offs = np.concatenate([[0], np.cumsum([m.size for m in mats])])
    outs = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])])
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(np.asarray(a, t))).to(dev)
    cost = d(np.concatenate([m.ravel() for m in mats]), np.float64)
    c_off, o_off = d(offs[:-1], np.int64), d(outs[:-1], np.int64)
    ld = d([m.shape[1] for m in mats], np.int32)
    nr, nc = d([m.shape[0] for m in mats], np.int32), ld
    col = torch.zeros(int(outs[-1]), device=dev, dtype=torch.int32)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    mr, mc = max(m.shape[0] for m in mats), max(m.shape[1] for m in mats)
    call = lambda: _lib.check(lib.cnl_lsap_batch_f64(cost.data_ptr(), c_off.data_ptr(), ld.data_ptr(), nr.data_ptr(), nc.data_ptr(), B, mr, mc,
                                                     col.data_ptr(), o_off.data_ptr(), status.data_ptr(), None), "cnl_lsap_batch_f64")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        t_dev.append(e0.elapsed_time(e1) * 1e3)
    t_cpu = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref = [linear_sum_assignment(m) for m in mats]
        t_cpu.append((time.perf_counter() - t0) * 1e6)
    got = col.cpu().numpy()
    same = all(np.array_equal(got[outs[b]:outs[b + 1]][r], c) for b, (r, c) in enumerate(ref)) and int(status.abs().sum()) == 0
    return t_dev, t_cpu, same


def run(case, S, steps, warmup, dev, bank_only):
    kw = CASES[case]
    frames = steps + warmup
    scenes = [tracker_ref.synth_sequence(s, frames=frames + 3 * (SCENES - 1), objects=kw["objects"] + s % 3, k=kw["k"]) for s in range(min(S, SCENES))]
    pick = lambda s, f: scenes[s % len(scenes)][f + 3 * ((s // len(scenes)) % SCENES)]
    data = [[torch.from_numpy(np.stack([pick(s, f)[j] for s in range(S)])).to(dev) for j in range(4)] for f in range(frames)]
    bank = cl.TrackerBank(num_streams=S, device=dev)
    trks = [] if bank_only else [cl.Tracker(device=dev) for _ in range(S)]
    torch.cuda.synchronize()
    t_bank, t_loop, d2h_bank, d2h_loop, sizes = [], [], [], [], []
    mats = None
    for f in range(frames):
        fr = data[f]
        t0 = time.perf_counter()
        bank.update_batch(*fr)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for s, trk in enumerate(trks):
            trk.update(fr[0][s], fr[1][s], fr[2][s], fr[3][s])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if f >= warmup:
            t_bank.append((t1 - t0) * 1e6)
            t_loop.append((t2 - t1) * 1e6)
            d2h_bank.append(bank.d2h_bytes)
            if trks:
                d2h_loop.append(sum(t.d2h_bytes for t in trks))
                sizes.append(np.mean([t.last_costs[0].shape for t in trks if t.last_costs is not None], axis=0))
        if trks and f == frames - 1:
            mats = [t.last_costs[0].copy() for t in trks if t.last_costs is not None]
    print(f"case {case} (k = {kw['k']})  S = {S:3d}  steps = {len(t_bank)}")
    print(f"  bank.update_batch          {pct(t_bank)}   d2h_bytes/step p50 {int(np.median(d2h_bank))}")
    if trks:
        n, T = np.mean(sizes, axis=0)
        same = all([t.track_id for t in bank[s].tracks] == [t.track_id for t in trks[s].tracks] for s in range(S))
        print(f"  loop over {S:3d} Tracker.update {pct(t_loop)}   d2h_bytes/step p50 {int(np.median(d2h_loop))}")
        spread = np.percentile(t_loop, 90) - np.percentile(t_loop, 10)
        gain = np.percentile(t_loop, 50) - np.percentile(t_bank, 50)
        print(f"  mean n x T = {n:.1f} x {T:.1f};  loop p50 - bank p50 = {gain:.1f} us, loop p90 - p10 = {spread:.1f} us;  "
              f"speed-up x{np.percentile(t_loop, 50) / np.percentile(t_bank, 50):.2f};  same track ids: {same}")
        t_dev, t_cpu, ok = lsap_alone(mats, dev)
        print(f"  assignment alone, {len(mats)} re-ID matrices of the last step: cnl_lsap_batch_f64 (one launch, HIP events) {pct(t_dev)}")
        print(f"                                                              scipy, one after the other       {pct(t_cpu)}   equal: {ok}")
    # the association pass alone on the frozen final state: cnl_track_streams_f32 + the synchronisation (no life cycle, no apply)
    lib = _lib.load()
    fr = data[-1]
    k, E = fr[3].shape[1], fr[3].shape[2]
    R = int(bank._off[S])
    T_max = int(np.max(np.diff(bank._off)))
    stride = int(lib.cnl_track_streams_record_bytes(k, T_max, 1))
    cur = torch.cuda.current_stream(dev)
    cur.synchronize()
    ctl = bank._ctl.np.view(np.int32)                    # the live list and trk_off of the state the bank is in NOW
    ctl[:S] = np.arange(S)
    ctl[S:2 * S + 1] = bank._off
    ws = torch.empty(int(lib.cnl_track_streams_workspace_bytes(S, k, T_max)), device=dev, dtype=torch.uint8)
    rec = _Mapped(S * stride)                            # a record block of this pass's own, sized for it
    lab = fr[1].contiguous()
    t_pass = []
    for i in range(60):
        t0 = time.perf_counter()
        _lib.check(lib.cnl_track_streams_f32(fr[3].data_ptr(), fr[0].data_ptr(), fr[2].data_ptr(), lab.data_ptr(), 1, S, S, bank._ctl.ptr, k, E, 0.3, 0.2, 0.5,
                                             bank._emb.data_ptr(), bank._box.data_ptr(), bank._ctl.ptr + 4 * S, R, T_max, 1, 0, 1, ws.data_ptr(),
                                             ws.numel(), rec.ptr, stride, ctypes.c_void_p(cur.cuda_stream)), "cnl_track_streams_f32")
        cur.synchronize()
        if i >= 10:
            t_pass.append((time.perf_counter() - t0) * 1e6)
    print(f"  association pass alone (two launches + the one synchronisation, R = {R} rows) {pct(t_pass)}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,32,64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--cases", default="readme,small")
    ap.add_argument("--bank-only", action="store_true")
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    print(f"track_streams_bench: {torch.cuda.get_device_name(0)}, steps = {a.steps} after {a.warmup} warm-up steps, wall time per step incl. the closing synchronisation")
    for case in a.cases.split(","):
        for S in (int(x) for x in a.streams.split(",")):
            run(case, S, a.steps, a.warmup, dev, a.bank_only)


if __name__ == "__main__":
    main()
