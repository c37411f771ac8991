"""Camera-motion compensation measured: the estimator's launches, the call, a torch-op restatement, and what the option costs a bank step.

    python tools/camera_motion_bench.py [--streams 32] [--reps 20] [--steps 40] [--warmup 10] [--parent-package DIR] [--out profiles/camera_motion_bench.txt]

S streams, half 1080 x 1920 and half 720 x 1280, two consecutive textured frames per stream (the second moved by a multiple of the coarse cell),
as packed RGB and as NV12 surfaces; the default rule (d = 4, 8 x 8 blocks of 16, radius 8).  Median (p10, p90) of `--reps`:
  (a) the three launches of cnl_camera_motion_u8, each alone, by HIP events (stages 1, 2, 4), with the bytes the coarse launch reads;
  (b) CameraMotion.update as a call: wall time from the call to the end of a closing synchronisation (records, the pinned upload, three launches);
  (c) the same rule in torch ops on the same frames — luma by a matmul, avg_pool2d, the windows gathered and unfolded into the 289 candidates
      of every block, SAD, argmin, median — and whether it finds the same shifts;
  (d) TrackerBank(lifecycle="device", use_kalman=True, kalman="device").update_batch at S streams, k = 300 (the scenes of tools/byte_bench.py),
      step by step alternating between a bank given camera_motion= and two banks without it: the option's one launch, and the run-to-run
      spread of two identical banks;
  (e) with --parent-package (a checkout of the parent commit with its library built in place): that checkout's bank, loaded under another
      module name, alternating with this tree's bank without the keyword in the same process.
"""
import argparse
import ctypes
import importlib.util
import os
import sys
import time
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "centernet-lightning_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from byte_bench import frames_for, pct          # noqa: E402  (the scenes and the percentile line of the BYTE bench)

SIZES = ((1080, 1920), (720, 1280))
D, GRID, B, R = 4, (8, 8), 16, 8
MARGIN = 32
LINES = []


def say(line=""):
    print(line)
    sys.stdout.flush()
    LINES.append(line)


def make_frames(S, dev):
    """-> (first, second, true shifts): per stream a contiguous [h, w, 3] frame and the same content moved by a multiple of D."""
    g = torch.Generator(device="cpu").manual_seed(0)
    canvases = {hw: torch.randint(0, 256, (hw[0] + 2 * MARGIN, hw[1] + 2 * MARGIN, 3), generator=g, dtype=torch.uint8).to(dev) for hw in SIZES}
    rng = np.random.default_rng(1)
    first, second, shifts = [], [], []
    for s in range(S):
        h, w = SIZES[s % 2]
        dx, dy = (int(v) * D for v in rng.integers(-R, R + 1, 2))
        c = canvases[(h, w)]
        first.append(c[MARGIN:MARGIN + h, MARGIN:MARGIN + w].contiguous())
        second.append(c[MARGIN - dy:MARGIN - dy + h, MARGIN - dx:MARGIN - dx + w].contiguous())
        shifts.append((dx, dy))
    return first, second, shifts


def to_nv12(frame):
    """A packed frame's luma (the estimator's rule) over a grey chroma plane: [h * 3 / 2, w]."""
    f = frame.to(torch.int32)
    y = ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).to(torch.uint8)
    return torch.cat([y, torch.full((frame.shape[0] // 2, frame.shape[1]), 128, dtype=torch.uint8, device=frame.device)])


def events(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return t


def wall(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return t


def stage_args(frames_a, frames_b, step, dev, _lib):
    """The operands of one cnl_camera_motion_u8 call on frames_b with frames_a's coarse planes as the previous ones (built here by stage 1)."""
    L, nb = len(frames_b), GRID[0] * GRID[1]
    planes = [[torch.empty((f.shape[0] * 2 // 3 if step == 1 else f.shape[0]) // D * (f.shape[1] // D), dtype=torch.uint8, device=dev) for f in frames_b]
              for _ in (0, 1)]
    keep = {"planes": planes}

    def table(frames, cur, prev):
        rec = np.zeros((L, 5), np.int64)
        for i, f in enumerate(frames):
            h = f.shape[0] * 2 // 3 if step == 1 else f.shape[0]
            rec[i, :3] = f.data_ptr(), cur[i].data_ptr(), prev[i].data_ptr() if prev is not None else 0
            rec[i, 3:].view(np.int32)[:3] = h, f.shape[1], f.stride(0)
        return torch.from_numpy(rec).to(dev)
    out = {"shift": torch.empty((L, 2), device=dev), "used": torch.empty(L, dtype=torch.int32, device=dev),
           "vectors": torch.empty((L, nb, 2), dtype=torch.int16, device=dev), "sad": torch.empty((L, nb), dtype=torch.int32, device=dev),
           "status": torch.empty(L, dtype=torch.int32, device=dev)}
    make = lambda t: _lib.CameraMotion(t.data_ptr(), None, None, *(out[k].data_ptr() for k in ("shift", "used", "vectors", "sad", "status")),
                                       L, 0, step, D, GRID[0], GRID[1], B, R, 4, 24, 4, 0)
    keep["tables"] = (table(frames_a, planes[0], None), table(frames_b, planes[1], planes[0]))
    return make(keep["tables"][0]), make(keep["tables"][1]), out, keep


def launches_alone(name, frames_a, frames_b, step, shifts, reps, dev, _lib):
    lib = _lib.load()
    stream = _lib.stream(dev)
    first, second, out, keep = stage_args(frames_a, frames_b, step, dev, _lib)
    _lib.check(lib.cnl_camera_motion_u8(ctypes.byref(first), 1, stream))
    rows = {}
    for label, stages in (("coarse luma", 1), ("block search", 2), ("aggregate", 4), ("all three", 7)):
        rows[label] = events(lambda: _lib.check(lib.cnl_camera_motion_u8(ctypes.byref(second), stages, stream)), reps)
    assert out["shift"].cpu().tolist() == [list(map(float, s)) for s in shifts] and int(out["used"].min()) == 64, "the planted shifts were not recovered"
    read = sum((f.shape[0] * 2 // 3 if step == 1 else f.shape[0]) * f.shape[1] * step for f in frames_b)
    say(f"(a) the launches alone, {name}, S = {len(frames_b)}, HIP events; the coarse launch reads {read / 1e6:.1f} MB")
    for label, v in rows.items():
        extra = f"   {read / np.median(v) / 1e6:7.2f} TB/s of frame bytes" if label == "coarse luma" else ""
        say(f"  {label:14s} {pct(v)}{extra}")


def torch_restatement(frames_a, frames_b):
    """The rule in torch ops, frames of one size batched -> shift [L, 2] (float32 SADs: exact below 2^24)."""
    weights = torch.tensor([77.0, 150.0, 29.0], device=frames_a[0].device)
    shift = torch.zeros((len(frames_b), 2), device=frames_a[0].device)
    side = 2 * R + 1
    for hw in SIZES:
        idx = [i for i, f in enumerate(frames_b) if tuple(f.shape[:2]) == hw]
        if not idx:
            continue
        planes = []
        for frames in (frames_a, frames_b):
            x = torch.stack([frames[i] for i in idx]).float()
            y = torch.floor((x @ weights + 128.0) / 256.0)
            planes.append(torch.floor(F.avg_pool2d(y[:, None], D) + 0.5)[:, 0])
        prev, cur = planes
        Hc, Wc = cur.shape[1:]
        ys = [R + (i * (Hc - 2 * R - B)) // (GRID[0] - 1) for i in range(GRID[0])]
        xs = [R + (i * (Wc - 2 * R - B)) // (GRID[1] - 1) for i in range(GRID[1])]
        wins = torch.stack([prev[:, y - R:y + B + R, x - R:x + B + R] for y in ys for x in xs], 1)          # [n, nb, W, W]
        blks = torch.stack([cur[:, y:y + B, x:x + B] for y in ys for x in xs], 1)                           # [n, nb, B, B]
        n, nb = wins.shape[:2]
        cand = F.unfold(wins.reshape(n * nb, 1, B + 2 * R, B + 2 * R), B)                                    # [n * nb, B * B, side^2]
        sad = (cand - blks.reshape(n * nb, B * B, 1)).abs().sum(1)
        best = sad.argmin(1)                            # candidate (wy, wx) = window offset; shift = R - offset
        sy, sx = R - best // side, R - best % side
        med = lambda v: v.reshape(n, nb).float().median(1).values
        shift[idx] = torch.stack([med(sx), med(sy)], 1) * D
    return shift


def load_package(directory, name):
    """The package of another checkout under another module name (its relative imports and its own lib/ directory come with it)."""
    pkg = os.path.join(directory, "centernet-lightning_amd", "centernet_lightning_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def alternate(banks, steps, data, warmup):
    """banks: name -> (bank, keyword arguments of a step).  Step by step, every bank in turn on the same detections."""
    times = {name: [] for name in banks}
    torch.cuda.synchronize()
    for f, fr in enumerate(data[:steps + warmup]):
        for name, (bank, kw) in banks.items():
            t0 = time.perf_counter()
            bank.update_batch(*fr, **kw)
            torch.cuda.synchronize()
            if f >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e6)
    return times


def paired(what, a, b, same_what, c, d):
    """The banks of a group alternate step by step on the same detections, so their times pair up per step.  The difference of interest is the
    median of the per-step differences a - b; the run-to-run spread is what the same statistic does between two IDENTICAL banks (c - d):
    their median and their p10 .. p90 range."""
    diff, same = np.asarray(a) - np.asarray(b), np.asarray(c) - np.asarray(d)
    lo, hi = np.percentile(same, 10), np.percentile(same, 90)
    med = float(np.median(diff))
    say(f"  per-step differences, {what}: median {med:+.1f} us (p10 {np.percentile(diff, 10):+.1f}, p90 {np.percentile(diff, 90):+.1f})")
    say(f"  per-step differences, {same_what} (identical banks: the spread): median {np.median(same):+.1f} us (p10 {lo:+.1f}, p90 {hi:+.1f})")
    say(f"  -> the median difference is {'within' if lo <= med <= hi else 'OUTSIDE'} the identical banks' p10 .. p90 range")


def luma_check(frame, say):
    """Where the torch-op restatement can leave the rule: its float32 matmul luma against the integer luma, on one frame."""
    f = frame.to(torch.int32)
    want = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    got = torch.floor((frame.float() @ torch.tensor([77.0, 150.0, 29.0], device=frame.device) + 128.0) / 256.0).to(torch.int32)
    bad = int((got != want).sum())
    say(f"      its matmul luma differs from the integer luma in {bad} of {want.numel()} pixels of stream 0's frame (largest difference {int((got - want).abs().max())})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-package", default=None, help="a checkout of the parent commit whose library is built in place, for part (e)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_motion_bench.txt"))
    a = ap.parse_args()
    import centernet_lightning_amd as cl
    from centernet_lightning_amd import _lib
    import tracker_ref                              # input recipe only
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "camera_motion_bench measures on a HIP device"
    dev = torch.device("cuda:0")
    S = a.streams
    say(f"command: python tools/camera_motion_bench.py --streams {S} --reps {a.reps} --steps {a.steps} --warmup {a.warmup}"
        + (" --parent-package <a checkout of the parent commit>" if a.parent_package else ""))
    say(f"{torch.cuda.get_device_name(0)}; S = {S} streams, alternately 1080 x 1920 and 720 x 1280; downscale {D}, grid {GRID}, block {B}, radius {R}; "
        f"median (p10, p90) of {a.reps}")
    first, second, shifts = make_frames(S, dev)
    formats = {"rgb": (first, second, 3), "nv12": ([to_nv12(f) for f in first], [to_nv12(f) for f in second], 1)}
    for name, (fa, fb, step) in formats.items():
        launches_alone(name, fa, fb, step, shifts, a.reps, dev, _lib)
    for name, (fa, fb, _) in formats.items():
        cm = cl.CameraMotion(S)
        flip = [0]

        def call():
            flip[0] ^= 1
            return cm.update(fb if flip[0] else fa, pixel_format=name)
        v = wall(call, a.reps)
        say(f"(b) CameraMotion.update, {name}, S = {S}: call + closing synchronisation   {pct(v)}")
    got = torch_restatement(first, second)
    wrong = sum(g != list(map(float, s)) for g, s in zip(got.cpu().tolist(), shifts))
    v = wall(lambda: torch_restatement(first, second), a.reps)
    say(f"(c) the rule in torch ops (matmul luma, avg_pool2d, unfold SAD, argmin, median), rgb, S = {S}: call + closing synchronisation   {pct(v)}"
        f"   streams whose shift differs from the planted one: {wrong} of {S}")
    if wrong:
        luma_check(second[0], say)

    data = frames_for(S, a.steps + a.warmup, dev, tracker_ref)
    kw = dict(num_streams=S, device=dev, lifecycle="device", use_kalman=True, kalman="device")
    shift = (torch.rand((S, 2), device=dev) - 0.5) * 0.01          # normalised boxes: half a percent of the frame
    banks = {"without (1)": (cl.TrackerBank(**kw), {}), "camera_motion=": (cl.TrackerBank(**kw), dict(camera_motion=shift)),
             "without (2)": (cl.TrackerBank(**kw), {})}
    times = alternate(banks, a.steps, data, a.warmup)
    say(f"(d) TrackerBank(lifecycle='device', kalman='device').update_batch, S = {S}, k = 300: step + closing synchronisation, {a.steps} steps after {a.warmup}")
    for name, t in times.items():
        say(f"  {name:16s} {pct(t)}")
    paired("camera_motion= - without (1)", times["camera_motion="], times["without (1)"], "without (2) - without (1)", times["without (2)"], times["without (1)"])
    if a.parent_package:
        parent = load_package(a.parent_package, "centernet_lightning_amd_parent")
        banks = {"this tree (1)": (cl.TrackerBank(**kw), {}), "parent commit": (parent.TrackerBank(**kw), {}), "this tree (2)": (cl.TrackerBank(**kw), {})}
        times = alternate(banks, a.steps, data, a.warmup)
        say(f"(e) the step without the keyword against the parent commit's package and library, alternating in this process")
        for name, t in times.items():
            say(f"  {name:16s} {pct(t)}")
        paired("this tree (1) - parent commit", times["this tree (1)"], times["parent commit"], "this tree (2) - this tree (1)", times["this tree (2)"],
               times["this tree (1)"])
    else:
        say("(e) no --parent-package: the parent commit was not measured in this run")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
