"""TEST INFRASTRUCTURE ONLY: the camera-motion rule of include/centernet_gfx950.h (cnl_camera_motion_u8) restated in numpy integers, the shift
of a track table (cnl_track_shift_f64) restated on tests/gate_ref.py's reference tracker, and a seeded shake scene.

`CameraMotion` has the product class's constructor and `update` / `reset`, on numpy frames: a 2-D uint8 array is a luma plane (the Y plane of a
YUV surface), a 3-D [h, w, C >= 3] array a packed frame.  Every quantity is an integer until the final float32 conversion, so the kernels are held
to equality.  It never touches a GPU.

The scene (`shake_scene`): a handful of small objects with constant velocity in front of a textured background, seen by a camera that jumps by
more than a box width for a few frames and returns.  `run_scene` tracks it with gate_ref.Tracker, with or without the shift applied to the
tracker's table and filter state before each update; `render` draws a frame of it (texture plus filled boxes)."""
import numpy as np

import gate_ref
from centernet_lightning_amd import _track_host as th


# ----------------------------------------------------------------------------------------------------------------------- the estimator's rule
def luma(frame):
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    if frame.ndim == 2:
        return frame.astype(np.int64)
    f = frame.astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def coarse(y, d):
    """Luma [h, w] -> the coarse plane [h // d, w // d]: the d x d sums, rounded to nearest by the shift."""
    Hc, Wc = y.shape[0] // d, y.shape[1] // d
    s = y[:Hc * d, :Wc * d].reshape(Hc, d, Wc, d).sum(axis=(1, 3))
    return (s + (d * d) // 2) >> (2 * (d.bit_length() - 1))


def block_starts(n, m, R, B):
    span = n - 2 * R - B
    return [R + span // 2] if m == 1 else [R + (i * span) // (m - 1) for i in range(m)]


def search(cur, prev, ys, xs, B, R):
    """-> (sad, sy, sx) int64 arrays over the blocks (row-major over ys x xs): the smallest key (SAD, |sy| + |sx|, sy, sx)."""
    H, W = cur.shape
    y0 = np.repeat(np.asarray(ys), len(xs)) - R         # block origins inside the interior [R, H - R) x [R, W - R)
    x0 = np.tile(np.asarray(xs), len(ys)) - R
    best = None
    for sy in range(-R, R + 1):
        for sx in range(-R, R + 1):
            diff = np.abs(cur[R:H - R, R:W - R] - prev[R - sy:H - R - sy, R - sx:W - R - sx])
            I = np.zeros((diff.shape[0] + 1, diff.shape[1] + 1), np.int64)
            I[1:, 1:] = diff.cumsum(0).cumsum(1)
            sad = I[y0 + B, x0 + B] - I[y0, x0 + B] - I[y0 + B, x0] + I[y0, x0]
            man = abs(sy) + abs(sx)
            if best is None:
                best = [sad, np.full_like(sad, man), np.full_like(sad, sy), np.full_like(sad, sx)]
                continue
            bs, bm, by, bx = best
            better = (sad < bs) | ((sad == bs) & ((man < bm) | ((man == bm) & ((sy < by) | ((sy == by) & (sx < bx))))))
            for arr, v in zip(best, (sad, man, sy, sx)):
                arr[better] = v[better] if isinstance(v, np.ndarray) else v
    return best[0], best[2], best[3]


class CameraMotion:
    def __init__(self, num_streams, downscale=4, grid=(8, 8), block=16, radius=8, min_texture=4, max_sad=24, min_blocks=4):
        self.num_streams, self.d, self.grid, self.B, self.R = num_streams, downscale, tuple(grid), block, radius
        self.min_texture, self.max_sad, self.min_blocks = min_texture, max_sad, min_blocks
        self.reset()

    def reset(self, stream=None):
        if stream is None:
            self.prev = [None] * self.num_streams       # each stream's previous coarse plane
        else:
            self.prev[stream] = None

    def update(self, frames, streams=None, boxes=None, count=None):
        live = list(range(self.num_streams)) if streams is None else list(streams)
        assert len(live) == len(frames)
        d, (gy, gx), B, R = self.d, self.grid, self.B, self.R
        nb, L = gy * gx, len(frames)
        out = {"shift": np.zeros((L, 2), np.float32), "used": np.zeros(L, np.int32), "vectors": np.zeros((L, nb, 2), np.int16),
               "sad": np.full((L, nb), -1, np.int32), "status": np.zeros(L, np.int32)}
        for i, (s, frame) in enumerate(zip(live, frames)):
            cur = coarse(luma(frame), d)
            prev, self.prev[s] = self.prev[s], cur
            Hc, Wc = cur.shape
            status = 0
            if prev is None or prev.shape != cur.shape:
                status |= 1
            if Hc < 2 * R + B or Wc < 2 * R + B:
                status |= 4
            votes_x, votes_y = [], []
            if status == 0:
                ys, xs = block_starts(Hc, gy, R, B), block_starts(Wc, gx, R, B)
                sad, sy, sx = search(cur, prev, ys, xs, B, R)
                for b in range(nb):
                    y0, x0 = ys[b // gx], xs[b % gx]
                    blk = cur[y0:y0 + B, x0:x0 + B]
                    m = (int(blk.sum()) + B * B // 2) // (B * B)
                    flat = int(np.abs(blk - m).sum()) < self.min_texture * B * B
                    bad = int(sad[b]) > self.max_sad * B * B
                    masked = False
                    if boxes is not None:
                        cx, cy = np.float32((x0 + B // 2) * d), np.float32((y0 + B // 2) * d)
                        n_live = boxes.shape[1] if count is None else min(max(int(count[i]), 0), boxes.shape[1])
                        for q in np.asarray(boxes[i][:n_live], np.float32):
                            if np.isfinite(q).all() and q[0] <= cx < q[2] and q[1] <= cy < q[3]:
                                masked = True
                    if flat or bad or masked:
                        continue
                    out["vectors"][i, b] = sx[b], sy[b]
                    out["sad"][i, b] = sad[b]
                    votes_x.append(int(sx[b]))
                    votes_y.append(int(sy[b]))
            n = len(votes_x)
            out["used"][i] = n
            if n < self.min_blocks:
                status |= 2
            else:
                out["shift"][i] = sorted(votes_x)[(n - 1) // 2] * d, sorted(votes_y)[(n - 1) // 2] * d
            out["status"][i] = status
        return out


def textured(rng, h, w, channels=3):
    """A frame-sized canvas of independent uint8 noise: every block of it is textured and no two windows of it match."""
    return rng.integers(0, 256, (h, w, channels) if channels else (h, w), dtype=np.uint8)


def window(canvas, h, w, margin, shift):
    """The h x w view of `canvas` whose content has moved by `shift` = (dx, dy) against the view at shift (0, 0); |shift| <= margin."""
    dx, dy = shift
    return np.ascontiguousarray(canvas[margin - dy:margin - dy + h, margin - dx:margin - dx + w])


# ----------------------------------------------------------------------------------------------------------------------- the tracker's shift
def shift_tracker(trk, dx, dy):
    """cnl_track_shift_f64 on gate_ref.Tracker: (dx, dy, dx, dy) (float32 values) added to the float32 box table, to the positions of the filter
    state and to every track's reported box (in the box's own type, float64 on the device)."""
    dx, dy = np.float32(dx), np.float32(dy)
    if not trk.tracks:
        return
    v = np.array([dx, dy, dx, dy], np.float32)
    trk.box = (trk.box + v).astype(np.float32)
    if trk.kx is not None:
        trk.kx = trk.kx.copy()
        trk.kx[:, :4] += v.astype(np.float64)
    for t in trk.tracks:
        t.bbox = np.asarray(t.bbox) + v.astype(np.asarray(t.bbox).dtype)


# ----------------------------------------------------------------------------------------------------------------------- the scene
H, W, MARGIN = 128, 160, 32
FRAMES, K, E = 20, 8, 8
JUMP = {8: (14, -10), 9: (16, -12), 10: (14, -10)}      # camera offset (dx, dy) in pixels during the shake; (0, 0) elsewhere
SIZE = (10.0, 14.0)                                     # objects' (width, height): the jump exceeds the width
ESTIMATOR = dict(downscale=2, grid=(4, 5), block=8, radius=8)        # shifts up to 16 pixels in steps of 2
TRACKER = dict(use_kalman=True, kalman="device", motion_gate=True)


def offsets():
    return [JUMP.get(f, (0, 0)) for f in range(FRAMES)]


def shake_scene(seed=3, objects=5):
    """-> (per frame (bboxes [K, 4] f32 in pixels, labels [K] i64, scores [K] f32, embeddings [K, E] f32), per frame {object: row}, world boxes
    [FRAMES, objects, 4]).  Object o is detection row o of every frame (scores descending); the other rows are clutter below every threshold."""
    rng = np.random.default_rng(seed)
    ident = rng.standard_normal((objects, E))
    start = np.stack([rng.uniform(24, W - 40, objects), rng.uniform(24, H - 40, objects)], 1)
    start[:, 0] = np.linspace(24, W - 40, objects)[rng.permutation(objects)]       # apart in x: the objects never overlap
    vel = rng.uniform(-0.6, 0.6, (objects, 2))
    dets, where, world = [], [], np.zeros((FRAMES, objects, 4))
    for f, (cx, cy) in enumerate(offsets()):
        boxes, scores, embs = [], [], []
        for o in range(objects):
            x, y = start[o] + f * vel[o]
            world[f, o] = x, y, x + SIZE[0], y + SIZE[1]
            boxes.append(world[f, o] + (cx, cy, cx, cy))
            scores.append(0.9 - 0.01 * o)
            embs.append(ident[o])
        while len(boxes) < K:
            c = rng.uniform(8, 100, 2)
            boxes.append([c[0], c[1], c[0] + 2, c[1] + 2])
            scores.append(0.05 * rng.random())
            embs.append(rng.standard_normal(E))
        dets.append((np.asarray(boxes, np.float32), np.zeros(K, np.int64), np.asarray(scores, np.float32), np.asarray(embs, np.float32)))
        where.append({o: o for o in range(objects)})
    return dets, where, world


def render(canvas, dets, f, objects=5):
    """Frame f of the scene: the background moved by the camera offset, every object a filled box of its own grey."""
    frame = window(canvas, H, W, MARGIN, offsets()[f]).copy()
    for o in range(objects):
        x1, y1, x2, y2 = (int(round(float(v))) for v in dets[f][0][o])
        frame[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = 40 + 40 * o
    return frame


def run_scene(dets, shifts):
    """gate_ref.Tracker over the scene; shifts: per frame (dx, dy) applied before the update, or None: uncompensated.
    -> (per frame {detection row: id of the track it was matched to} — a detection that starts a track is not in it —, per frame
    [(track id, state)] of all tracks after the update).  The scene's confident detections are rows 0 .. objects - 1 in score order, so a
    kept-detection row of `last_matches` is the detection row."""
    trk = gate_ref.Tracker(**TRACKER)
    ids, states = [], []
    for f, det in enumerate(dets):
        if shifts is not None:
            shift_tracker(trk, *shifts[f])
        old = [t.track_id for t in trk.tracks]
        trk.update(*det)
        ids.append({int(row): old[t] for row, t in trk.last_matches})
        states.append([(t.track_id, t.state) for t in trk.tracks])
    return ids, states
