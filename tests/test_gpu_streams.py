"""GPU: the video, tracking and evaluation APIs away from the default stream.  Every comparison is an equality of bytes against the same
call on the default stream; no kernel is re-derived here (the other files hold them to their rules).

Part 2, one side stream while the default stream is busy: stream_probe.run_on_side (its docstring has the protocol).  Besides the bytes,
`busy` is asserted: when the call's own stream has been synchronised, the filler on the default stream must still be running, so the call
neither waited for the default stream nor synchronised the device.  A call that really does synchronise the device would be named in
DEVICE_WIDE with the line that does it (at most three entries, none of the entries the README calls sync-free); the table is empty.

Part 3, stateful objects whose stream changes between calls.  Tracker / TrackerBank: frame t under streams[t % 2] with NO wait_stream and
no synchronisation by the test (TrackTable's stream rule is what is under test), and TrackTable.apply wrapped so that APPLY_DELAY_MS of
filler sit in front of every table update: the previous frame's update is really still pending when the next frame starts.  Track.embedding
/ Track.kf read under the OTHER stream right after a frame.  CocoEvaluator / LossMeter / HeadTrainer + SGD: call i under streams[i % 2]
with the ordinary torch protocol (wait_stream on the previous stream).  Two independent objects on two streams, interleaved.

Nothing here switches off a synchronisation of the package to show that the tests would notice: with the mapped index lists overwritten
under a running kernel the gather indices could leave the old table.  What shows it safely: the attribute reads (valid table memory only;
before TrackTable.read_row they were unordered against the pending update), the `busy` assertion — which did find two waits, see below —
and tests/test_streams_host.py.

Measured on the MI355X ("Streams away from the default stream", has the same figures):
  filler unit            0.120 ms (one 2048^3 fp32 torch.mm; median of 10 event timings of 20 units)
  R                      12.  Started at 4.  No correct call came out not busy for a filler too short, but the rule asks for twice the largest
                         (side run with the filler queued) / t_call: 5.8 (CocoEvaluator.update, 2.15 / 0.37 ms; detect_tiled 12.5 / 2.8 = 4.4,
                         detect_multiscale 13.3 / 3.4 = 3.9: the side run builds the plans of its own stream).  Every call that small runs under
                         the 50 ms floor, at most 13.3 ms of it; the longest side run with a longer filler, HeadTrainer's, took 15.7 of 1000 ms.
  what was NOT the call  (a) Tracker.reset() / TrackerBank.reset() at the START of the side run: it finishes the stream of the last update, by
                         design, and that was the default stream with the filler on it — all eight tracker cases came out not busy, 44 ms side
                         run under a 50 ms filler; the reset now closes the run.  (b) One fresh stream in four shares the default stream's
                         hardware queue and waits for the filler in hardware (43 ms for a merge_soft): stream_probe.runs_beside_default.
  APPLY_DELAY_MS         30: the host time of one default-stream frame is 0.16 .. 0.31 ms (medians over 8 .. 32 frames), ten times that is 3 ms.
  wall time per test     at most 1.7 s (detect_frames, whose warm-up packs the weights; the four-step SGD test; CocoEvaluator's first update);
                         every tracker test 0.07 .. 0.30 s; the file 16 s.
"""
import time
import warnings

import numpy as np
import pytest
import torch

import byte_ref
import letterbox_ref
import ref_cpu
import soft_nms_ref
import stream_probe
import tiled_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd._track_host import TrackTable
from centernet_lightning_amd.letterbox import letterbox_uint8
from stream_probe import filler, fresh_side_stream, run_on_side, same, to_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# call name -> "file:line, why" for a call that synchronises the whole device by design: bytes only are asserted for it.
DEVICE_WIDE = {}
SYNC_FREE = ("letterbox_uint8", "letterbox_yuv420", "tile_uint8", "merge_tiles", "merge_soft", "crop_detections", "draw_detections",
             "mirror_append_uint8", "flip_merge", "CocoEvaluator.update")
APPLY_DELAY_MS = 30.0

CANVAS = (64, 96)
SIZES = [(37, 53), (64, 64), (7, 5), (120, 90), (1, 1)]
YUV_SIZES = [(36, 52), (64, 64), (120, 88)]
FILL = (7, 8, 9, 10)


def test_the_device_wide_table_is_short_and_names_no_sync_free_entry():
    assert len(DEVICE_WIDE) <= 3
    assert not any(name.startswith(entry) for name in DEVICE_WIDE for entry in SYNC_FREE)


def check_side(name, call, warm):
    got, ref, busy = run_on_side(call, warm)
    t_call, fill, t_side, _ = stream_probe.TIMES[-1]
    print(f"{name}: t_call {t_call:.2f} ms, filler {fill:.0f} ms, side run {t_side:.2f} ms, busy {busy}")
    assert same(got, ref), f"{name}: the side stream's bytes differ from the default stream's"
    if not any(name.startswith(entry) for entry in DEVICE_WIDE):
        assert busy, f"{name}: the default stream had drained when the call's stream was synchronised (filler {fill:.0f} ms, side run {t_side:.2f} ms)"
    return ref


# ============================================================================================================ part 2: frame-level calls
def rgb_frames(seed, sizes=SIZES, C=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, C), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in sizes]


def yuv_surfaces(seed, sizes=YUV_SIZES):
    """Form (a) of yuv.py: one [h * 3 / 2, w] tensor per frame, read as NV12 or as I420."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h * 3 // 2, w), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in sizes]


def _letterbox(C):
    def build(seed):
        frames = rgb_frames(seed, C=C)

        def call():
            canvas, geom = letterbox_uint8(frames, *CANVAS, fill=FILL)
            return canvas, [list(f) for f in geom.frames]
        return call
    return build


def _letterbox_yuv(layout):
    def build(seed):
        frames = yuv_surfaces(seed)

        def call():
            canvas, geom = cl.letterbox_yuv420(frames, *CANVAS, layout=layout, fill=FILL)
            return canvas, [list(f) for f in geom.frames]
        return call
    return build


def _tile(seed):
    frames = rgb_frames(seed, [(150, 200), (64, 64)])

    def call():
        views, geom = cl.tile_uint8(frames, 64, 64, overlap=0.2, full_frame=True, fill=FILL)
        return views, geom.merge_table, geom.first_view, [list(v) for v in geom.views]
    return call


MERGE_SIZES = [(150, 200), (64, 64)]


def _merge(kind):
    """40 candidates per view with planted duplicates (soft_nms_ref.planted_candidates, the recipe of tests/test_gpu_tiles.py's
    random_candidates), on the views of tile_uint8 (merge_tiles) or on two scales per frame (merge_soft).  No model is involved."""
    if kind == "tiles":
        rec, ffv, _ = tiled_ref.view_records(MERGE_SIZES, 64, 64, 0.2, True, letterbox_ref.geometry)
    else:
        rec, ffv = soft_nms_ref.scale_records(MERGE_SIZES, 2, canvas=64)

    def build(seed):
        boxes, scores, labels = soft_nms_ref.planted_candidates(np.random.default_rng(seed), rec, ffv, 40, n_objects=10)
        b, s, lab = (torch.from_numpy(a).to(DEV) for a in (boxes, scores, labels))
        geom = cl.TileGeometry.from_records(rec, ffv, DEV)
        if kind == "tiles":
            return lambda: cl.merge_tiles(b, s, lab, geom, max_detections=50, score_threshold=0.1)
        return lambda: cl.merge_soft(b, s, lab, geom, method=kind, max_detections=50, score_threshold=0.05)
    return build


def frame_boxes(rng, sizes, k=9):
    """k boxes inside each frame, float32 [N, k, 4]; slot 7 is not finite; the scores put slot 5 under the threshold (a dead slot)."""
    boxes = np.zeros((len(sizes), k, 4), np.float32)
    for n, (h, w) in enumerate(sizes):
        x0, y0 = rng.uniform(0, w * 0.6, k), rng.uniform(0, h * 0.6, k)
        boxes[n] = np.stack([x0, y0, x0 + rng.uniform(1, w * 0.4 + 1, k), y0 + rng.uniform(1, h * 0.4 + 1, k)], 1)
    boxes[:, 7, 2] = np.inf
    scores = rng.uniform(0.5, 1.0, (len(sizes), k)).astype(np.float32)
    scores[:, 5] = 0.1
    return torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV)


def _crops(pixel_format):
    def build(seed):
        sizes = SIZES if pixel_format == "rgb" else YUV_SIZES
        frames = rgb_frames(seed, sizes) if pixel_format == "rgb" else yuv_surfaces(seed, sizes)
        boxes, scores = frame_boxes(np.random.default_rng(seed), sizes)
        return lambda: cl.crop_detections(frames, boxes, size=(32, 16), scores=scores, score_threshold=0.3, pad=0.1, fill=FILL[:3],
                                          pixel_format=pixel_format)
    return build


def _draw(pixel_format):
    def build(seed):
        sizes = SIZES if pixel_format == "rgb" else YUV_SIZES
        frames = rgb_frames(seed, sizes) if pixel_format == "rgb" else yuv_surfaces(seed, sizes)
        rng = np.random.default_rng(seed)
        boxes, scores = frame_boxes(rng, sizes)
        labels = torch.from_numpy(rng.integers(0, 12, (len(sizes), 9))).to(DEV)
        numbers = torch.from_numpy(rng.integers(-1, 120, (len(sizes), 9)).astype(np.int32)).to(DEV)
        return lambda: cl.draw_detections(frames, boxes, labels=labels, scores=scores, score_threshold=0.3, numbers=numbers, fill_alpha=64,
                                          pixel_format=pixel_format, inplace=False)
    return build


def _mirror(seed):
    canvas = torch.randint(0, 256, (2, 5, 67, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).to(DEV)
    return lambda: cl.mirror_append_uint8(canvas)


def _flip_merge(seed):
    g = torch.Generator().manual_seed(seed)
    outs = cl.TrackingOutput(*(torch.randn((4, C, 5, 67), generator=g).to(DEV).contiguous(memory_format=torch.channels_last) for C in (3, 4, 8)))
    assert "box_2d" in outs._fields
    return lambda: list(cl.flip_merge(outs, 2))


FRAME_CALLS = {
    "letterbox_uint8": _letterbox(3), "letterbox_uint8 C=4": _letterbox(4),
    "letterbox_yuv420 nv12": _letterbox_yuv("nv12"), "letterbox_yuv420 i420": _letterbox_yuv("i420"),
    "tile_uint8": _tile,
    "merge_tiles": _merge("tiles"), "merge_soft gaussian": _merge("gaussian"), "merge_soft hard": _merge("hard"),
    "crop_detections rgb": _crops("rgb"), "crop_detections nv12": _crops("nv12"),
    "draw_detections rgb": _draw("rgb"), "draw_detections nv12": _draw("nv12"),
    "mirror_append_uint8": _mirror, "flip_merge": _flip_merge,
}


@pytest.mark.parametrize("name", list(FRAME_CALLS))
def test_frame_level_call_on_a_side_stream(name):
    assert any(name.startswith(entry) for entry in SYNC_FREE)
    check_side(name, FRAME_CALLS[name](1), FRAME_CALLS[name](1001))


# ============================================================================================================ part 2: model-level calls
DET = {"model": {"backbone": {"name": "resnet18"}, "neck": {"name": "simple"}, "output_heads": {"heatmap": {"num_classes": 4}, "box_2d": {}}}}
TRACK = {"model": {"task": "tracking", "backbone": {"name": "resnet18"},
                   "neck": {"name": "fpn", "upsample_channels": [256, 128, 64], "upsample_type": "nearest", "conv_type": "normal"},
                   "output_heads": {"heatmap": {"num_classes": 2, "init_bias": -2.19}, "box_2d": {"init_bias": 10},
                                    "reid": {"init_bias": 0, "max_track_ids": 800}}}}
TRAIN = {"model": {"backbone": {"name": "resnet18"}, "neck": {"name": "simple"},
                   "output_heads": {"heatmap": {"num_classes": 3, "width": 32, "depth": 2}, "box_2d": {"width": 32, "depth": 2}}}}
_WEIGHTS, _MODELS = {}, {}


def new_model(which):
    """A model of the config on the device that has not run yet; the weights are synthesised once per config."""
    torch.manual_seed(0)
    model = cl.build_centernet({"DET": DET, "TRACK": TRACK, "TRAIN": TRAIN}[which])
    if which not in _WEIGHTS:
        _WEIGHTS[which] = ref_cpu.synth_state_dict(model.state_dict(), seed=0, calib_shape=(2, 3, 64, 64))
    model.load_state_dict(_WEIGHTS[which])
    return model.to(DEV)


def model_of(which):
    if which not in _MODELS:
        _MODELS[which] = new_model(which)
    return _MODELS[which]


MODEL_CALLS = {
    "detect_frames": ("DET", lambda m, f: m.detect_frames(f, *CANVAS, num_detections=20), SIZES),
    "detect_frames flip_test": ("DET", lambda m, f: m.detect_frames(f, *CANVAS, num_detections=20, flip_test=True), SIZES),
    "detect_tiled": ("DET", lambda m, f: m.detect_tiled(f, tile=(64, 64), batch=8, num_detections=20, max_detections=30, score_threshold=0.0),
                     [(150, 200), (64, 64)]),
    "detect_multiscale": ("DET", lambda m, f: m.detect_multiscale(f, scales=(0.5, 1.0), height=64, width=64, num_detections=20, max_detections=30), SIZES),
    "detect_frames tracking": ("TRACK", lambda m, f: m.detect_frames(f, *CANVAS, num_detections=20), SIZES),
}


@pytest.mark.parametrize("name", list(MODEL_CALLS))
def test_model_level_call_on_a_side_stream(name):
    which, fn, sizes = MODEL_CALLS[name]
    model = model_of(which)
    frames, other = rgb_frames(2, sizes), rgb_frames(1002, sizes)
    check_side(name, lambda: fn(model, frames), lambda: fn(model, other))


FIRST_FORWARD_T_CALL_MS = 60.0          # by hand (no warm-up here): both forwards of the ResNet-18, packing and two plans included, took 44 ms


def test_first_forward_of_a_fresh_model_on_a_side_stream():
    """The path through the lazily built shared buffers (split weights, row-pair weights, the up2 pack, the folded out_conv weights): built on
    the first stream, read by the second stream's plan.  The second forward is ordered behind the first by wait_stream and nothing else."""
    fresh, plain = new_model("DET"), new_model("DET")
    g = torch.Generator().manual_seed(3)
    x1, x2 = (torch.rand((2, 3, 64, 64), generator=g).to(DEV) for _ in range(2))
    first, second = fresh_side_stream(), fresh_side_stream()
    torch.cuda.synchronize()
    default = torch.cuda.default_stream()
    fill = min(stream_probe.R * FIRST_FORWARD_T_CALL_MS, stream_probe.Filler.CAP_MS)
    filler().queue(default, fill)
    t0 = time.perf_counter()
    with torch.cuda.stream(first):
        out1 = fresh.get_encoded_outputs(x1)
    second.wait_stream(first)
    with torch.cuda.stream(second):
        out2 = fresh.get_encoded_outputs(x2)
        first.synchronize()
        second.synchronize()
        busy = not default.query()
        t_side = (time.perf_counter() - t0) * 1e3
        got = to_host([out1, out2])
    torch.cuda.synchronize()
    assert len({key[-1] for key in fresh._engine.plans}) == 2            # one plan per stream
    ref = to_host([plain.get_encoded_outputs(x1), plain.get_encoded_outputs(x2)])
    print(f"first forward: filler {fill:.0f} ms, both forwards {t_side:.2f} ms, busy {busy}")
    assert same(got, ref)
    assert busy, f"the default stream had drained (filler {fill:.0f} ms, both forwards {t_side:.2f} ms)"


# ============================================================================================================ part 2: evaluators, training side
def coco_batch(seed, N=4, k=20, K=5):
    """Integer-grid boxes, scores in eighths (ties), ground truths that are jittered copies of some detections; targets as the host list."""
    rng = np.random.default_rng(seed)
    xy, wh = rng.integers(0, 60, (N, k, 2)), rng.integers(4, 40, (N, k, 2))
    boxes = np.concatenate([xy, xy + wh], 2).astype(np.float32)
    scores = (rng.integers(1, 8, (N, k)) / 8).astype(np.float32)
    labels = rng.integers(0, K, (N, k))
    targets = []
    for n in range(N):
        g = int(rng.integers(0, 7))
        pick = rng.permutation(k)[:g]
        gt = np.concatenate([xy[n, pick] + rng.integers(-2, 3, (g, 2)), wh[n, pick] + rng.integers(-2, 3, (g, 2))], 1).astype(np.float64)
        targets.append({"boxes": gt.reshape(g, 4), "labels": labels[n, pick].astype(np.int64)})
    return {"bboxes": torch.from_numpy(boxes).to(DEV), "scores": torch.from_numpy(scores).to(DEV), "labels": torch.from_numpy(labels).to(DEV)}, targets


def coco_result(ev):
    metrics = ev.get_metrics()
    return metrics, ev.precision, ev.recall, ev.num_images


def test_coco_evaluator_on_a_side_stream():
    ev = cl.CocoEvaluator(num_classes=5, device=DEV)

    def build(seed):
        batches = [coco_batch(seed), coco_batch(seed + 1)]

        def call():
            ev.reset()
            for preds, targets in batches:
                ev.update(preds, targets)
            return coco_result(ev)
        return call
    check_side("CocoEvaluator.update x 2 + get_metrics", build(1), build(1001))


def test_coco_update_alone_is_sync_free_on_a_side_stream():
    """update by itself (get_metrics ends in a download, which synchronises its own stream only): the records it appended."""
    ev = cl.CocoEvaluator(num_classes=5, device=DEV)

    def build(seed):
        batches = [coco_batch(seed), coco_batch(seed + 1)]

        def call():
            ev.reset()
            for preds, targets in batches:
                ev.update(preds, targets)
            state = ev.state()
            return [state[k] for k in sorted(state)]
        return call
    check_side("CocoEvaluator.update", build(1), build(1001))


def test_mot_evaluator_on_a_side_stream():
    from test_gpu_mot_eval import world_sequence
    frames = world_sequence(1, 12, 8, 10)
    moved = [(gt + np.array([1.0, 0.0, 0.0, 0.0]), gid, pred, pid) for gt, gid, pred, pid in frames]      # the same shapes, other values

    def build(fr):
        def call():
            ev = cl.MotEvaluator(device=DEV)
            ev.update([f[2] for f in fr], [f[3] for f in fr], [f[0] for f in fr], [f[1] for f in fr], sequence="a")
            return ev.get_metrics()
        return call
    check_side("MotEvaluator.get_metrics", build(frames), build(moved))


def loss_batches(shift):
    from test_gpu_loss import case, device_targets
    out = []
    for name in ("edges", "tiles"):
        heat, box, _, padded, _ = case(name)
        out.append(({"heatmap": torch.from_numpy(heat + np.float32(shift)).to(DEV).contiguous(memory_format=torch.channels_last),
                     "box_2d": torch.from_numpy(box + np.float32(shift)).to(DEV).contiguous(memory_format=torch.channels_last)}, device_targets(padded)))
    return out


LOSS_SETTINGS = dict(stride=4, box_loss="giou", box_loss_weight=5.0)


def test_loss_meter_on_a_side_stream():
    def build(shift):
        batches = loss_batches(shift)

        def call():
            meter = cl.LossMeter(**LOSS_SETTINGS)
            for outputs, targets in batches:
                meter.update(outputs, targets)
            return meter.get_metrics()
        return call
    check_side("LossMeter", build(0.0), build(0.25))


ONE = 1 << 16


def pixel_plan():
    """Every operation of pixel_batch and NONE, one canvas each (tests/pixel_ref.py states their rules)."""
    plan = cl.PixelPlan.empty(7)
    plan.set_motion_blur(1, 15, (0, 3), (14, 9))
    plan.set_sharpen(2, 0.5)
    plan.set_posterize(3, 3)
    plan.set_solarize(4, 100)
    plan.set_equalize(5)
    plan.set_filter(6, [(15, -15, ONE)])
    return plan.check()


def test_pixel_batch_on_a_side_stream():
    plan = pixel_plan()

    def build(seed):
        canvas = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (7, 40, 52, 3), dtype=np.uint8)).to(DEV)
        return lambda: cl.pixel_batch(canvas, plan, hole_fill=(9, 200, 77))
    check_side("pixel_batch", build(1), build(1001))


def train_targets(N=2, H=64, W=96):
    rng = np.random.default_rng(5)
    out = []
    for n in range(N):
        m = 3 + n
        wh = rng.uniform(10, 30, (m, 2))
        xy = rng.uniform(0, 1, (m, 2)) * (np.array([W, H]) - wh)
        out.append({"boxes": np.concatenate([xy, wh], 1), "labels": rng.integers(0, 2, m).astype(np.int64)})
    return out


def features(seed, C):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2, C, 16, 24), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)


def train_step(trainer, criterion, f, targets):
    trainer.zero_grad(set_to_none=True)
    loss = criterion(trainer.forward_features(f), targets)
    loss["total"].backward()
    return loss


def test_head_trainer_forward_and_backward_on_a_side_stream():
    model = model_of("TRAIN")
    C = model.neck.out_channels
    assert C == 64
    trainer, criterion, targets = model.head_trainer(), model.criterion(), train_targets()

    def build(seed):
        f = features(seed, C)

        def call():
            loss = train_step(trainer, criterion, f, targets)
            return {k: p.grad.clone() for k, p in trainer.heads.named_parameters()}, loss["total"].detach()
        return call
    grads, _ = check_side("HeadTrainer forward + backward", build(1), build(1001))
    assert len(grads) == len(list(trainer.parameters())) and all(float(g.abs().max()) > 0 for g in grads.values())


# ============================================================================================================ trackers
MODES = {"plain": dict(), "kalman_host": dict(use_kalman=True, kalman="host"), "kalman_device": dict(use_kalman=True, kalman="device"),
         "byte": dict(low_threshold=0.1)}
FRAMES, K, E, S = 8, 70, 32, 3


def quiet(cls, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(*a, device=DEV, **kw)


def sequence(seed, objects=6):
    return byte_ref.synth_occlusion(seed, objects=objects, k=K, emb_dim=E)[0][:FRAMES]


def on_device(frames):
    return [tuple(torch.from_numpy(a).to(DEV) for a in fr) for fr in frames]


def mixed_inputs(frames):
    """Device tensors on even frames, the numpy arrays themselves on odd ones (both input paths of update)."""
    return [tuple(torch.from_numpy(a).to(DEV) for a in fr) if t % 2 == 0 else fr for t, fr in enumerate(frames)]


def track_fields(tracks):
    return {"ids": [t.track_id for t in tracks], "states": [(t.state.name, t.birth_age, t.inactive_age) for t in tracks],
            "labels": [int(t.label) for t in tracks], "boxes": [np.array(t.bbox) for t in tracks]}


def table_rows(table, n):
    """The live rows of the device table, cloned on the current stream: the stream of the update that wrote them."""
    return {name: getattr(table, name)[:n].clone() if n and getattr(table, name) is not None else None for name in ("emb", "box", "kx", "kP")}


def pairs(matches):
    return None if matches is None else [tuple(int(v) for v in p) for p in matches]


def tracker_snapshot(trk):
    return {**track_fields(trk.tracks), "matches": pairs(trk.last_matches), "low": pairs(trk.last_low_matches), "next": trk.next_track_id,
            **table_rows(trk._table, len(trk.tracks))}


def bank_snapshot(bank):
    return {"streams": [{**track_fields(bank[s].tracks), "next": bank[s].next_track_id} for s in range(bank.num_streams)],
            "matches": [pairs(m) for m in bank.last_matches], "low": [pairs(m) for m in bank.last_low_matches], "off": bank._off.copy(),
            **table_rows(bank._table, int(bank._off[bank.num_streams]))}


def stack(frames, as_torch=True):
    cols = [np.stack([fr[j] for fr in frames]) for j in range(4)]
    return [torch.from_numpy(c).to(DEV) for c in cols] if as_torch else cols


@pytest.mark.parametrize("mode", list(MODES))
def test_tracker_on_a_side_stream(mode):
    trk = quiet(cl.Tracker, **MODES[mode])

    def build(seed):
        data = on_device(sequence(seed))

        def call():
            out = []
            for fr in data:
                trk.update(*fr)
                out.append(tracker_snapshot(trk))
            trk.reset()          # at the END, under the stream of the frames: reset() finishes the stream of the last update, by design, and
            return out           # at the start of the side run that would be the default stream with the filler on it
        return call
    ref = check_side(f"Tracker.update {mode}", build(7), build(1007))
    assert len(ref[-1]["ids"]) >= 6 and (mode != "byte" or any(len(s["low"]) for s in ref))


@pytest.mark.parametrize("mode", list(MODES))
def test_tracker_bank_on_a_side_stream(mode):
    bank = quiet(cl.TrackerBank, num_streams=S, **MODES[mode])

    def build(seed):
        seqs = [sequence(seed + s, objects=3 + s) for s in range(S)]
        data = [stack([seqs[s][t] for s in range(S)]) for t in range(FRAMES)]

        def call():
            out = []
            for fr in data:
                bank.update_batch(*fr)
                out.append(bank_snapshot(bank))
            bank.reset()         # (at the end: see test_tracker_on_a_side_stream)
            return out
        return call
    ref = check_side(f"TrackerBank.update_batch {mode}", build(20), build(1020))
    assert int(ref[-1]["off"][S]) >= 3 + 4 + 5 and (mode != "byte" or any(len(m) for s in ref for m in s["low"]))


# ============================================================================================================ part 3: the stream changes between frames
def slow_apply():
    """TrackTable.apply behind APPLY_DELAY_MS of filler on the stream it launches on: the table update stays pending after the frame returns."""
    original = TrackTable.apply

    def apply(self, src_trk, src_det, d_emb, d_box, E, smoothing_factor, cur, keep_emb=None):
        filler().queue(cur, APPLY_DELAY_MS)
        return original(self, src_trk, src_det, d_emb, d_box, E, smoothing_factor, cur, keep_emb)
    return apply


HOST_GAPS = []          # host time of one frame of the default-stream runs (ms): what APPLY_DELAY_MS has to exceed


def run_tracker(trk, data, streams=None, after_frame=None):
    """Frame t under streams[t % 2] (None: the default stream), nothing between the frames -> the snapshots, still on the device."""
    out = []
    for t, fr in enumerate(data):
        t0 = time.perf_counter()
        with torch.cuda.stream(streams[t % 2]) if streams else torch.cuda.stream(torch.cuda.default_stream()):
            trk.update(*fr)
            out.append(tracker_snapshot(trk))
        if streams is None:
            HOST_GAPS.append((time.perf_counter() - t0) * 1e3)
        if after_frame is not None:
            after_frame(t, trk)
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_tracker_whose_stream_changes_every_frame(mode, monkeypatch):
    data = mixed_inputs(sequence(7))
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        m.setattr(TrackTable, "apply", slow_apply())
        got = run_tracker(quiet(cl.Tracker, **MODES[mode]), data, [torch.cuda.Stream(), torch.cuda.Stream()])
        torch.cuda.synchronize()
        got = to_host(got)
    ref = run_tracker(quiet(cl.Tracker, **MODES[mode]), data)
    torch.cuda.synchronize()
    ref = to_host(ref)
    for t in range(FRAMES):
        assert same(got[t], ref[t]), (mode, t)
    assert len(ref[-1]["ids"]) >= 6 and (mode != "byte" or any(len(s["low"]) for s in ref))
    print(f"host time of a default-stream frame: median {np.median(HOST_GAPS):.3f} ms over {len(HOST_GAPS)} frames")


def run_bank(bank, seqs, streams=None):
    """Eight steps over S streams with one partial step (step 3: streams 2 and 0, in that order) and reset(stream=1) before step 6."""
    nxt, out = [0] * S, []
    for t in range(FRAMES):
        with torch.cuda.stream(streams[t % 2]) if streams else torch.cuda.stream(torch.cuda.default_stream()):
            if t == 6:
                bank.reset(stream=1)
                nxt[1] = 0
            live = [2, 0] if t == 3 else list(range(S))
            bank.update_batch(*stack([seqs[s][nxt[s]] for s in live], as_torch=t % 2 == 0), streams=None if len(live) == S else live)
            for s in live:
                nxt[s] += 1
            out.append(bank_snapshot(bank))
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_tracker_bank_whose_stream_changes_every_step(mode, monkeypatch):
    seqs = [sequence(20 + s, objects=3 + s) for s in range(S)]
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        m.setattr(TrackTable, "apply", slow_apply())
        got = run_bank(quiet(cl.TrackerBank, num_streams=S, **MODES[mode]), seqs, [torch.cuda.Stream(), torch.cuda.Stream()])
        torch.cuda.synchronize()
        got = to_host(got)
    ref = run_bank(quiet(cl.TrackerBank, num_streams=S, **MODES[mode]), seqs)
    torch.cuda.synchronize()
    ref = to_host(ref)
    for t in range(FRAMES):
        assert same(got[t], ref[t]), (mode, t)
    assert int(ref[-1]["off"][S]) >= 3 + 4 + 5
    before, after = ref[5]["streams"][1]["states"], ref[6]["streams"][1]["states"]          # reset(stream=1): its tracks were born again in step 6
    assert before and all(s[0] != "UNCONFIRMED" for s in before) and after and all(s[0] == "UNCONFIRMED" for s in after)


@pytest.mark.parametrize("mode", ["plain", "kalman_device"])
def test_track_attributes_read_under_the_other_stream(mode, monkeypatch):
    """Right after a frame, with the table update still queued on the frame's stream, Track.embedding (and Track.kf.x / .P in device mode)
    are read under the other stream: they are the rows of the FINISHED update (TrackTable.read_row)."""
    data = on_device(sequence(7))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    reads = {"side": [], "default": []}

    def read(where, cur):
        def after_frame(t, trk):
            with torch.cuda.stream(cur(t)):
                row = {"embedding": [x.embedding for x in trk.tracks]}
                if mode == "kalman_device":
                    row["x"], row["P"] = [x.kf.x for x in trk.tracks], [x.kf.P for x in trk.tracks]
            reads[where].append(row)
        return after_frame
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        m.setattr(TrackTable, "apply", slow_apply())
        run_tracker(quiet(cl.Tracker, **MODES[mode]), data, streams, read("side", lambda t: streams[(t + 1) % 2]))
        torch.cuda.synchronize()
    run_tracker(quiet(cl.Tracker, **MODES[mode]), data, None, read("default", lambda t: torch.cuda.default_stream()))
    torch.cuda.synchronize()
    for t in range(FRAMES):
        assert len(reads["default"][t]["embedding"]) >= (6 if t else 1)
        assert same(reads["side"][t], reads["default"][t]), (mode, t)
    for row in reads["default"][-1]["embedding"]:
        assert row.dtype == np.float32 and row.shape == (E,) and np.abs(row).max() > 0


# ============================================================================================================ part 3: the ordinary torch protocol
def alternate(calls, read_out):
    """calls[i] under streams[i % 2] after streams[i % 2].wait_stream(streams[(i - 1) % 2]); read_out on the default stream behind the last."""
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, call in enumerate(calls):
        if i:
            streams[i % 2].wait_stream(streams[(i - 1) % 2])
        with torch.cuda.stream(streams[i % 2]):
            call()
    torch.cuda.default_stream().wait_stream(streams[(len(calls) - 1) % 2])
    with torch.cuda.stream(torch.cuda.default_stream()):
        return to_host(read_out())


def one_stream(calls, read_out):
    for call in calls:
        call()
    return to_host(read_out())


def test_coco_evaluator_whose_stream_changes_between_updates():
    batches = [coco_batch(30 + i) for i in range(4)]
    torch.cuda.synchronize()
    a, b = cl.CocoEvaluator(num_classes=5, device=DEV), cl.CocoEvaluator(num_classes=5, device=DEV)
    got = alternate([lambda p=p, t=t: a.update(p, t) for p, t in batches], lambda: coco_result(a))
    torch.cuda.synchronize()
    ref = one_stream([lambda p=p, t=t: b.update(p, t) for p, t in batches], lambda: coco_result(b))
    assert same(got, ref) and ref[3] == 16 and max(ref[0].values()) > 0


def test_loss_meter_whose_stream_changes_between_updates():
    batches = loss_batches(0.0) + loss_batches(0.25)
    torch.cuda.synchronize()
    a, b = cl.LossMeter(**LOSS_SETTINGS), cl.LossMeter(**LOSS_SETTINGS)
    got = alternate([lambda o=o, t=t: a.update(o, t) for o, t in batches], a.get_metrics)
    torch.cuda.synchronize()
    ref = one_stream([lambda o=o, t=t: b.update(o, t) for o, t in batches], b.get_metrics)
    assert same(got, ref) and a.num_batches == b.num_batches == 4


def test_head_trainer_sgd_whose_stream_changes_between_steps():
    targets = train_targets()
    feats = [features(40 + i, 64) for i in range(4)]
    torch.cuda.synchronize()

    def steps(model):
        trainer, criterion = model.head_trainer(), model.criterion()
        opt = torch.optim.SGD(trainer.parameters(), lr=0.001)
        losses = []

        def step(f):
            losses.append(train_step(trainer, criterion, f, targets)["total"].detach())
            opt.step()
        return [lambda f=f: step(f) for f in feats], lambda: ({k: p.detach().clone() for k, p in trainer.heads.named_parameters()}, list(losses))
    start = {k: v.clone() for k, v in new_model("TRAIN").heads.state_dict().items()}
    got = alternate(*steps(new_model("TRAIN")))
    torch.cuda.synchronize()
    ref = one_stream(*steps(new_model("TRAIN")))
    assert same(got, ref)
    assert any(not torch.equal(ref[0][k], start[k].cpu()) for k in ref[0])          # the steps moved the parameters


# ============================================================================================================ part 3: two objects, two streams
def test_two_trackers_interleaved_on_two_streams():
    kw = dict(use_kalman=True, kalman="device", low_threshold=0.1)
    data = [on_device(sequence(seed)) for seed in (1, 2)]
    torch.cuda.synchronize()
    trks = [quiet(cl.Tracker, **kw) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [[], []]
    for t in range(FRAMES):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                trks[i].update(*data[i][t])
                got[i].append(tracker_snapshot(trks[i]))
    torch.cuda.synchronize()
    got = to_host(got)
    for i in range(2):
        ref = to_host(run_tracker(quiet(cl.Tracker, **kw), data[i]))
        torch.cuda.synchronize()
        assert same(got[i], ref), i
        assert any(len(s["low"]) for s in ref) and len(ref[-1]["ids"]) >= 6


def test_two_coco_evaluators_interleaved_on_two_streams():
    batches = [[coco_batch(50 + 10 * i + j) for j in range(3)] for i in range(2)]
    torch.cuda.synchronize()
    evs = [cl.CocoEvaluator(num_classes=5, device=DEV) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for j in range(3):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                evs[i].update(*batches[i][j])
    got = []
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            got.append(coco_result(evs[i]))
    torch.cuda.synchronize()
    for i in range(2):
        lone = cl.CocoEvaluator(num_classes=5, device=DEV)
        for preds, targets in batches[i]:
            lone.update(preds, targets)
        assert same(got[i], coco_result(lone)), i
    assert not same(got[0], got[1])
