"""GPU: sliced inference — tile_uint8 (the tile gather through cnl_letterbox_bilinear_u8), cnl_merge_tiles_f32 and CenterNet.detect_tiled.

Every comparison is EXACT.  Tile pixels are compared byte for byte with the frame crop (tests/tiled_ref.crop_view) and the full-frame view
with tests/letterbox_ref.expected_canvas; the merge's float outputs are compared as uint32 bit patterns with tests/tiled_ref.merge_ref,
the numpy float32 restatement of the rule in include/centernet_gfx950.h."""
import os

import numpy as np
import pytest
import torch

import bench
import letterbox_ref
import tiled_ref
import centernet_lightning_amd as cl

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")
F = np.float32
FILL = (114, 7, 201)
SCORES = np.array([0.05, 0.15, 0.3, 0.5, 0.7, 0.9], dtype=F)       # few values: ties are frequent; 0.05 fails the default threshold


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_merge_equal(got, want, what=""):
    """got: the dict of merge_tiles (tensors) or numpy arrays; want: merge_ref's dict."""
    g = {key: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for key, v in got.items()}
    assert np.array_equal(g["count"], want["count"]), (what, g["count"].tolist(), want["count"].tolist())
    assert g["count"].dtype == np.int32 and g["source"].dtype == np.int32 and g["labels"].dtype == np.int64
    assert np.array_equal(g["source"], want["source"]), (what, np.argwhere(g["source"] != want["source"])[:5].tolist())
    assert np.array_equal(g["labels"], want["labels"]), what
    assert same_bits(g["scores"], want["scores"]), what
    assert same_bits(g["bboxes"], want["bboxes"]), (what, np.argwhere(g["bboxes"] != want["bboxes"])[:5].tolist())


def gpu_merge(boxes, scores, labels, records, ffv, K_out, **kw):
    geom = cl.TileGeometry.from_records(records, ffv, "cuda")
    return cl.merge_tiles(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), geom,
                          max_detections=K_out, **kw)


def random_candidates(rng, records, ffv, k, n_objects=60, pass_all=False):
    """Candidates that overlap often: each frame has n_objects true boxes; every candidate of a view is one of them seen through the
    view (jittered by a few pixels, cut by the view's window as the decode of a tile would see it), in view pixels."""
    V = len(records)
    boxes = np.zeros((V, k, 4), dtype=F)
    for n in range(len(ffv) - 1):
        fw, fh = records[ffv[n]][0], records[ffv[n]][1]
        cx, cy = rng.uniform(0, fw, n_objects), rng.uniform(0, fh, n_objects)
        bw, bh = rng.uniform(20, 260, n_objects), rng.uniform(20, 260, n_objects)
        for v in range(ffv[n], ffv[n + 1]):
            _, _, x0, y0, pl, pt, sx, sy = records[v]
            o = rng.integers(0, n_objects, k)
            j = rng.uniform(-6, 6, (k, 4)) * (rng.random((k, 1)) < 0.7)                      # 30 % exact repeats of the object's box
            fb = np.stack([cx[o] - bw[o] / 2, cy[o] - bh[o] / 2, cx[o] + bw[o] / 2, cy[o] + bh[o] / 2], axis=1) + j
            vb = np.stack([(fb[:, 0] - x0) * sx + pl, (fb[:, 1] - y0) * sy + pt, (fb[:, 2] - x0) * sx + pl, (fb[:, 3] - y0) * sy + pt], axis=1)
            boxes[v] = np.clip(vb, -8, 520).astype(F)
    scores = rng.choice(SCORES[1:] if pass_all else SCORES, (V, k)).astype(F)
    labels = rng.integers(0, 3, (V, k)).astype(np.int64)
    return boxes, scores, labels


def frames_1080p(n):
    return tiled_ref.view_records([(1080, 1920)] * n, 512, 512, 0.2, True, letterbox_ref.geometry)[:2]


# ----------------------------------------------------------------------------- tile pixels
def test_tiles_are_the_frame_crops_and_the_full_view_is_the_letterbox():
    rng = np.random.default_rng(11)
    sizes = [(1080, 1920), (720, 1280), (300, 400), (513, 1000)]
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in sizes]
    wide = rng.integers(0, 256, (720, 1400, 3), dtype=np.uint8)
    host[1] = wide[:, 57:1337]                                                               # a row-strided view, read in place
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in host]
    dev[1] = torch.from_numpy(wide).cuda()[:, 57:1337]
    assert not dev[1].is_contiguous()
    views, geom = cl.tile_uint8(dev, 512, 512, 0.2, True, FILL)
    rec, ffv, want_views = tiled_ref.view_records(sizes, 512, 512, 0.2, True, letterbox_ref.geometry)
    assert geom.views == want_views and geom.frame_first_view == ffv == [0, 16, 23, 25, 32] and geom.sizes == sizes
    assert tuple(views.shape) == (32, 512, 512, 3) and views.dtype == torch.uint8 and tuple(geom.table.shape) == (32, 5)
    want_table = np.zeros((32, 8), dtype=np.int32)
    want_table[:, :6] = [r[:6] for r in rec]
    want_table[:, 6:] = np.array([r[6:] for r in rec], dtype=F).view(np.int32)
    assert np.array_equal(geom.merge_table.cpu().numpy(), want_table) and geom.first_view.cpu().tolist() == ffv
    got = views.cpu().numpy()
    compared = 0
    for v, (n, y0, x0, th, tw) in enumerate(want_views):
        if v == ffv[n + 1] - 1:                                                              # the full-frame view
            want = letterbox_ref.expected_canvas([np.ascontiguousarray(host[n])], 512, 512, FILL)[0][0]
        else:
            want = tiled_ref.crop_view(host[n], y0, x0, th, tw, 512, 512, FILL)
            if th < 512 or tw < 512:                                                         # the padding is the fill
                assert (got[v, th:] == np.array(FILL, dtype=np.uint8)).all() and (got[v, :, tw:] == np.array(FILL, dtype=np.uint8)).all()
        bad = np.argwhere(got[v] != want)
        assert len(bad) == 0, (v, (n, y0, x0, th, tw), bad[:5].tolist())
        compared += want.size
    print(f"tile gather: {compared} bytes compared, all equal")
    # without the full view, other tile sizes and channel counts; a 4-D tensor is N equal frames
    u8 = torch.from_numpy(rng.integers(0, 256, (2, 700, 1300, 4), dtype=np.uint8)).cuda()
    views, geom = cl.tile_uint8(u8, 608, 1088, 0.5, False, (1, 2, 3, 4))
    grid = tiled_ref.tile_grid_ref(700, 1300, 608, 1088, 0.5)
    assert len(geom) == 2 * len(grid) and geom.frame_first_view == [0, len(grid), 2 * len(grid)]
    for v, (n, y0, x0, th, tw) in enumerate(geom.views):
        assert np.array_equal(views[v].cpu().numpy(), tiled_ref.crop_view(u8[n].cpu().numpy(), y0, x0, th, tw, 608, 1088, (1, 2, 3, 4)))


# ----------------------------------------------------------------------------- the merge against the restated rule
@pytest.mark.parametrize("N", [1, 3, 32])
def test_merge_equals_the_restated_rule(N):
    rec, ffv = frames_1080p(N)
    assert ffv[1] == 16
    rng = np.random.default_rng(100 + N)
    boxes, scores, labels = random_candidates(rng, rec, ffv, 100)
    if N >= 3:
        scores[ffv[1]:ffv[2]] = rng.choice(np.array([0.01, 0.05, 0.1], dtype=F), (16, 100))    # frame 1: nothing exceeds 0.1
    for metric in ("iou", "ios"):
        for class_aware in (True, False):
            for t in (0.3, 0.5, 0.7):
                want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, 300, match_threshold=t, metric=cl.tiles.METRICS[metric], class_aware=class_aware)
                got = gpu_merge(boxes, scores, labels, rec, ffv, 300, match_threshold=t, match_metric=metric, class_aware=class_aware)
                assert_merge_equal(got, want, (N, metric, class_aware, t))
                print(f"merge N={N} {metric} class_aware={class_aware} t={t}: counts {want['count'].min()}..{want['count'].max()} identical")
                if N >= 3:
                    assert want["count"][1] == 0 and (got["source"][1] == -1).all() and (got["scores"][1] == 0).all() and (got["bboxes"][1] == 0).all()
    # fewer outputs than survivors, and a cap that bites: every frame has ~1300 candidates above the threshold
    for K_out, cap in ((7, 4096), (300, 1000), (64, 100), (300, 1), (2000, 4096)):      # the last: the walk is never cut short
        want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, K_out, max_candidates=cap)
        assert (scores[:16] > F(0.1)).sum() > 1000
        assert_merge_equal(gpu_merge(boxes, scores, labels, rec, ffv, K_out, max_candidates=cap), want, (N, K_out, cap))


def test_merge_of_a_frame_that_leaves_the_lds_sort():
    sizes = [(2160, 3840), (1080, 1920), (300, 400)]
    rec, ffv, _ = tiled_ref.view_records(sizes, 512, 512, 0.2, True, letterbox_ref.geometry)
    assert ffv == [0, 61, 77, 79]                                                            # 6100 candidates in frame 0: the sort pads to 8192 keys
    rng = np.random.default_rng(5)
    boxes, scores, labels = random_candidates(rng, rec, ffv, 100, n_objects=400, pass_all=True)
    scores[:61].reshape(-1)[rng.choice(6100, 100, replace=False)] = F(0.05)
    assert (scores[:61] > F(0.1)).sum() == 6000
    for cap, K_out in ((8192, 300), (8192, 1000), (4096, 300), (16384, 300)):
        want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, K_out, max_candidates=cap, match_threshold=0.5)
        got = gpu_merge(boxes, scores, labels, rec, ffv, K_out, max_candidates=cap, match_threshold=0.5)
        assert_merge_equal(got, want, (cap, K_out))
        print(f"large frame: cap {cap}, K_out {K_out}: counts {want['count'].tolist()}")
    # nothing suppresses anything: the walk reaches far into the sorted list
    want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, 7000, max_candidates=8192, match_threshold=1.5)
    assert want["count"][0] == 6000
    assert_merge_equal(gpu_merge(boxes, scores, labels, rec, ffv, 7000, max_candidates=8192, match_threshold=1.5), want, "no match")


def test_a_frame_in_a_batch_of_32_equals_the_frame_alone():
    rec, ffv = frames_1080p(32)
    boxes, scores, labels = random_candidates(np.random.default_rng(77), rec, ffv, 100)
    batch = {key: v.cpu().numpy() for key, v in gpu_merge(boxes, scores, labels, rec, ffv, 300, match_metric="ios").items()}
    for n in range(32):
        s = slice(ffv[n], ffv[n + 1])
        alone = gpu_merge(boxes[s], scores[s], labels[s], rec[s], [0, 16], 300, match_metric="ios")
        assert_merge_equal(alone, {key: v[n:n + 1] for key, v in batch.items()}, n)
    # frames without views, and no views at all
    got = gpu_merge(boxes[:16], scores[:16], labels[:16], rec[:16], [0, 0, 16, 16], 50)
    want = tiled_ref.merge_ref(boxes[:16], scores[:16], labels[:16], rec[:16], [0, 0, 16, 16], 50)
    assert want["count"][0] == 0 and want["count"][2] == 0 and want["count"][1] > 0
    assert_merge_equal(got, want, "empty frames")
    got = gpu_merge(boxes[:0], scores[:0], labels[:0], [], [0, 0], 50)
    assert got["count"].tolist() == [0] and (got["source"] == -1).all()


def test_planted_duplicates_leave_one_box_per_object():
    rec, ffv = frames_1080p(1)
    # objects inside the overlap of tiles 0 and 1 (x 410..512, y 0..512), of tiles 0 and 5 (y 410..512) and of 0, 1, 5, 6
    objects = [(420, 100, 470, 160), (430, 300, 500, 380), (100, 420, 180, 500), (415, 415, 505, 505), (440, 20, 480, 60)]
    seen_by = [(0, 1), (0, 1), (0, 5), (0, 1, 5, 6), (1, 0)]
    boxes, scores, labels = np.zeros((16, 100, 4), F), np.zeros((16, 100), F), np.zeros((16, 100), np.int64)
    rng = np.random.default_rng(1)
    rank = [0] * 16
    for i, (box, tiles) in enumerate(zip(objects, seen_by)):
        for t in tiles:
            x0, y0 = rec[t][2], rec[t][3]
            shift = rng.uniform(-0.9, 0.9, 4)                                                # the same object, shifted by less than a pixel
            boxes[t, rank[t]] = (np.array(box) - np.array([x0, y0, x0, y0]) + shift).astype(F)
            scores[t, rank[t]] = F(0.9 - 0.1 * i - 0.01 * t)
            labels[t, rank[t]] = i % 2
            rank[t] += 1
    for metric in ("iou", "ios"):
        got = gpu_merge(boxes, scores, labels, rec, ffv, 300, match_metric=metric)
        assert_merge_equal(got, tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, 300, metric=cl.tiles.METRICS[metric]), metric)
        assert got["count"].tolist() == [len(objects)]
        kept = got["bboxes"][0, :len(objects)].cpu().numpy()
        for i, box in enumerate(objects):                                                    # in score order: object i is row i
            assert np.abs(kept[i] - np.array(box)).max() < 1.0, (i, kept[i])


def test_nan_boxes_nan_scores_and_signed_zero_scores_follow_the_rule():
    rec, ffv = frames_1080p(1)
    rng = np.random.default_rng(9)
    boxes, scores, labels = random_candidates(rng, rec, ffv, 100)
    flat = scores.reshape(-1)
    flat[rng.choice(1600, 300, replace=False)] = F("nan")                                    # never take part
    zeros = rng.choice(1600, 400, replace=False)
    flat[zeros[:200]], flat[zeros[200:]] = F(0.0), F(-0.0)                                   # one score: ordered by candidate number
    bf = boxes.reshape(-1)
    bf[rng.choice(bf.size, 200, replace=False)] = F("nan")                                   # a NaN coordinate maps to 0
    for st, K_out in ((-1.0, 2000), (0.1, 300), (-0.0, 2000)):
        want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, K_out, score_threshold=st, match_threshold=0.7)
        got = gpu_merge(boxes, scores, labels, rec, ffv, K_out, score_threshold=st, match_threshold=0.7)
        assert_merge_equal(got, want, st)
        assert not np.isnan(want["bboxes"]).any() and not np.isnan(want["scores"]).any()
        print(f"NaN / signed zero, threshold {st}: count {want['count'].tolist()}")
    want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, 2000, score_threshold=-1.0, match_threshold=0.7)
    kept_zero = want["source"][0][(want["scores"][0] == 0) & (want["source"][0] >= 0)]
    assert len(kept_zero) > 20 and (np.diff(kept_zero) > 0).all()                            # -0 and +0 interleave by candidate number


# ----------------------------------------------------------------------------- end to end
def build(config):
    torch.manual_seed(0)
    return bench.synthetic_weights_(cl.build_centernet(os.path.join(CONFIGS, bench.CONFIGS[config]))).cuda()


@pytest.mark.parametrize("config", ["simple", "tracking"])
def test_detect_tiled_equals_the_pipeline_assembled_by_hand(config):
    model = build(config)
    tracking = config == "tracking"
    sizes = [(1080, 1920), (720, 1280), (300, 400), (513, 1000)]
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for (h, w) in sizes]
    rec, ffv, views = tiled_ref.view_records(sizes, 512, 512, 0.2, True, letterbox_ref.geometry)
    # by hand, from calls that existed before: crop with torch, letterbox_uint8 for the full view, forward_uint8, gather_*, merge_ref
    canvas = []
    for v, (n, y0, x0, th, tw) in enumerate(views):
        if v == ffv[n + 1] - 1:
            canvas.append(model.letterbox_uint8([frames[n]], 512, 512, fill=FILL)[0][0])
        else:
            t = torch.empty((512, 512, 3), dtype=torch.uint8, device="cuda")
            t[...] = torch.tensor(FILL, dtype=torch.uint8, device="cuda")
            t[:th, :tw] = frames[n][y0:y0 + th, x0:x0 + tw]
            canvas.append(t)
    out = model.forward_uint8(torch.stack(canvas))
    dets = (model.gather_tracking2d if tracking else model.gather_detection2d)(out, num_detections=100, nms_kernel=3, normalize_bbox=False)
    d = {key: v.cpu().numpy() for key, v in dets.items()}
    for kw in ({}, {"match_metric": "ios", "match_threshold": 0.3, "class_aware": False, "max_detections": 40}):
        want = tiled_ref.merge_ref(d["bboxes"], d["scores"], d["labels"], rec, ffv, kw.get("max_detections", 300), score_threshold=0.1,
                                   match_threshold=kw.get("match_threshold", 0.5), metric=cl.tiles.METRICS[kw.get("match_metric", "iou")],
                                   class_aware=kw.get("class_aware", True))
        print(f"detect_tiled {config} {kw}: {(d['scores'] > F(0.1)).sum()} candidates above 0.1, counts {want['count'].tolist()}")
        for batch in (32, 5):
            got = model.detect_tiled(frames, fill=FILL, batch=batch, **kw)
            assert set(got) == ({"bboxes", "labels", "scores", "count", "embeddings"} if tracking else {"bboxes", "labels", "scores", "count"})
            g = {key: v.cpu().numpy() for key, v in got.items()}
            assert np.array_equal(g["count"], want["count"]) and g["count"].dtype == np.int32, (batch, g["count"], want["count"])
            assert np.array_equal(g["labels"], want["labels"]) and same_bits(g["scores"], want["scores"]) and same_bits(g["bboxes"], want["bboxes"]), batch
            if tracking:
                emb = np.zeros(want["source"].shape + (d["embeddings"].shape[-1],), dtype=F)
                for n in range(len(sizes)):
                    m = want["count"][n]
                    emb[n, :m] = d["embeddings"][ffv[n]:ffv[n + 1]].reshape(-1, emb.shape[-1])[want["source"][n, :m]]
                assert same_bits(g["embeddings"], emb), batch
