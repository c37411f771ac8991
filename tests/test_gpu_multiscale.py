"""GPU: the multi-scale test — cnl_merge_soft_f32 against the numpy restatement of its rule (tests/soft_nms_ref.py) and
CenterNet.detect_multiscale against the pipeline assembled by hand.

Methods "hard" and "linear" are compared bit for bit.  "gaussian" goes through exp, which the device and numpy round differently by a
couple of float64 ulp: boxes, labels, sources and counts are equal, and a score, which is the float64 working score rounded once to
float32, differs by at most one float32 ulp (a relative 1e-13 moves a float32 rounding by one step at most).  That the picks themselves
cannot differ is the margin tests/test_multiscale_host.py proves for every case used here."""
import os

import numpy as np
import pytest
import torch

import bench
import soft_nms_ref as ref
import centernet_lightning_amd as cl

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")
F = np.float32
METHODS = ("hard", "linear", "gaussian")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulps(a, b):
    """The distance of two float32 arrays in steps of the float32 grid (sign-magnitude bits mapped to a line)."""
    line = lambda x: np.where(bits(x).astype(np.int64) < 2 ** 31, bits(x).astype(np.int64), 2 ** 31 - bits(x).astype(np.int64))
    return int(np.abs(line(a) - line(b)).max()) if a.size else 0


def assert_soft_equal(got, want, exact, what=""):
    """got: the dict of merge_soft (tensors); want: soft_merge_ref's.  -> the largest score difference in float32 ulp."""
    g = {key: v.cpu().numpy() for key, v in got.items()}
    assert g["count"].dtype == np.int32 and g["source"].dtype == np.int32 and g["labels"].dtype == np.int64
    assert np.array_equal(g["count"], want["count"]), (what, g["count"].tolist(), want["count"].tolist())
    assert np.array_equal(g["source"], want["source"]), (what, np.argwhere(g["source"] != want["source"])[:5].tolist())
    assert np.array_equal(g["labels"], want["labels"]), what
    assert np.array_equal(bits(g["bboxes"]), bits(want["bboxes"])), (what, np.argwhere(g["bboxes"] != want["bboxes"])[:5].tolist())
    worst = ulps(g["scores"], want["scores"])
    print(f"{what}: counts {want['count'].tolist()}, scores differ by at most {worst} float32 ulp")
    if exact:
        assert np.array_equal(bits(g["scores"]), bits(want["scores"])), what
    else:
        assert want["margin"] >= ref.MIN_MARGIN, (what, want["margin"])      # (proved beforehand on the host; see the module docstring)
        assert worst <= 1, (what, worst)
    return worst


def gpu_soft(boxes, scores, labels, records, ffv, K_out, **kw):
    geom = cl.TileGeometry.from_records(records, ffv, "cuda")
    return cl.merge_soft(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), geom, max_detections=K_out, **kw)


# ----------------------------------------------------------------------------- the merge against the restated rule
@pytest.mark.parametrize("N,S,seed", ref.RANDOM_CASES)
def test_soft_merge_equals_the_restated_rule(N, S, seed):
    boxes, scores, labels, rec, ffv = ref.random_case(N, S, seed)
    assert boxes.shape[:2] == (N * S, 100)
    for method in METHODS:
        want = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, ref.RANDOM_K_OUT, method=method, **ref.RANDOM_KW)
        got = gpu_soft(boxes, scores, labels, rec, ffv, ref.RANDOM_K_OUT, method=method, **ref.RANDOM_KW)
        assert_soft_equal(got, want, method != "gaussian", f"N={N} S={S} {method}")


@pytest.mark.parametrize("name", sorted(ref.edge_cases()))
def test_edge_sizes_and_values_follow_the_rule(name):
    boxes, scores, labels, rec, ffv, K_out, kw = ref.edge_cases()[name]
    for method in METHODS:
        want = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, K_out, method=method, **kw)
        assert_soft_equal(gpu_soft(boxes, scores, labels, rec, ffv, K_out, method=method, **kw), want, method != "gaussian", f"{name} {method}")
    if name == "M=257":                                                   # more rows than candidates, and the other parameters of the decay
        for kw2 in ref.DECAY_VARIANTS:
            kw3 = dict(kw, **kw2)
            want = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 1000, **kw3)
            assert_soft_equal(gpu_soft(boxes, scores, labels, rec, ffv, 1000, **kw3), want, kw3["method"] != "gaussian", f"{name} {kw2}")


def test_the_hard_method_is_merge_tiles_bit_for_bit():
    boxes, scores, labels, rec, ffv = ref.random_case(3, 5, 77)
    geom = cl.TileGeometry.from_records(rec, ffv, "cuda")
    dev = [torch.from_numpy(a).cuda() for a in (boxes, scores, labels)]
    cut = 0
    for (t, st, K_out) in ((0.5, 0.05, 300), (0.5, 0.05, 40), (0.3, 0.0, 100), (0.7, 0.5, 7), (0.5, 0.05, 1)):
        hard = cl.merge_tiles(*dev, geom, max_detections=K_out, score_threshold=st, match_threshold=t, match_metric="iou")
        soft = cl.merge_soft(*dev, geom, method="hard", iou_threshold=t, score_threshold=st, max_detections=K_out)
        assert set(hard) == set(soft)
        for key in hard:
            a, b = hard[key].cpu().numpy(), soft[key].cpu().numpy()
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (key, t, st, K_out)
        full = cl.merge_tiles(*dev, geom, max_detections=600, score_threshold=st, match_threshold=t, match_metric="iou")["count"].cpu().numpy()
        cut += int((full > K_out).sum())
        print(f"hard t={t} score>{st} K_out={K_out}: counts {hard['count'].tolist()} (uncut {full.tolist()}) identical")
    assert cut >= 6                                                       # K_out cut the list in most of these


def test_a_frame_in_a_batch_of_8_equals_the_frame_alone():
    sizes = (ref.FRAME_SIZES * 3)[:8]
    rec, ffv = ref.scale_records(sizes, 3)
    boxes, scores, labels = ref.planted_candidates(np.random.default_rng(88), rec, ffv, 100)
    for method in METHODS:
        batch = {key: v.cpu().numpy() for key, v in gpu_soft(boxes, scores, labels, rec, ffv, 100, method=method, score_threshold=0.05).items()}
        for n in range(8):
            s = slice(ffv[n], ffv[n + 1])
            alone = gpu_soft(boxes[s], scores[s], labels[s], rec[s], [0, 3], 100, method=method, score_threshold=0.05)
            for key, v in alone.items():
                a = v.cpu().numpy()
                assert np.array_equal(a.view(np.uint8), batch[key][n:n + 1].view(np.uint8)), (method, n, key)
    # frames without views, and no views at all
    got = gpu_soft(boxes[:3], scores[:3], labels[:3], rec[:3], [0, 0, 3, 3], 50, method="linear")
    want = ref.soft_merge_ref(boxes[:3], scores[:3], labels[:3], rec[:3], [0, 0, 3, 3], 50, method="linear")
    assert want["count"][0] == 0 and want["count"][2] == 0 and want["count"][1] > 0
    assert_soft_equal(got, want, True, "empty frames")
    got = gpu_soft(boxes[:0], scores[:0], labels[:0], [], [0, 0], 50)
    assert got["count"].tolist() == [0] and (got["source"] == -1).all() and (got["scores"] == 0).all()


def test_two_overlapping_objects_seen_at_three_scales_both_survive_the_soft_merge():
    boxes, scores, labels, rec, ffv = ref.planted_pair()
    hard = gpu_soft(boxes, scores, labels, rec, ffv, 10, method="hard", iou_threshold=0.5, score_threshold=0.05)
    assert hard["count"].tolist() == [1] and hard["source"][0, 0].item() == 0              # IoU 0.6 > 0.5: the second object is gone
    want = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 10, method="gaussian", sigma=0.5, score_threshold=0.05)
    soft = gpu_soft(boxes, scores, labels, rec, ffv, 10, method="gaussian", sigma=0.5, score_threshold=0.05)
    assert_soft_equal(soft, want, False, "planted pair")
    got = {key: v.cpu().numpy() for key, v in soft.items()}
    assert got["count"][0] >= 2 and got["source"][0, :2].tolist() == [0, 1]                # both objects, the best view of each
    objects = np.array([[20, 30, 120, 130], [45, 30, 145, 130]], dtype=F)
    assert np.abs(got["bboxes"][0, :2] - objects).max() < 1.0
    assert got["scores"][0, 0] == F(0.9) and 0.05 < got["scores"][0, 1] < F(0.8)
    assert abs(float(got["scores"][0, 1]) - float(want["scores64"][0, 1])) <= 2.0 ** -25   # the decayed score the restatement gives
    assert abs(float(want["scores64"][0, 1]) - 0.8 * np.exp(-0.36 / 0.5)) < 0.01           # 0.8 x exp(-0.6^2 / 0.5), up to the jitter


# ----------------------------------------------------------------------------- end to end
def build(config):
    torch.manual_seed(0)
    return bench.synthetic_weights_(cl.build_centernet(os.path.join(CONFIGS, bench.CONFIGS[config]))).cuda()


@pytest.mark.parametrize("config", ["simple", "tracking"])
def test_detect_multiscale_equals_the_pipeline_assembled_by_hand(config):
    model = build(config)
    tracking = config == "tracking"
    sizes = [(90, 160), (120, 100)]
    scales, fill = (0.5, 1.0, 1.5), (114, 7, 201)
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for (h, w) in sizes]
    assert cl.multiscale_sizes(128, 128, scales) == [(64, 64), (128, 128), (192, 192)]
    for flip_test in ((False, True) if not tracking else (False,)):
        # by hand: per scale letterbox_uint8 -> forward_uint8 -> the decode; the records written out; merge_soft
        parts, rec = [], {}
        for s, side in enumerate((64, 128, 192)):
            canvas, geom = model.letterbox_uint8(frames, side, side, fill=fill)
            out = model.forward_uint8(canvas, flip_test=flip_test)
            parts.append((model.gather_tracking2d if tracking else model.gather_detection2d)(out, num_detections=50, nms_kernel=3, normalize_bbox=False))
            for n, (h, w, nh, nw, pt, pl) in enumerate(geom.frames):
                rec[(n, s)] = (w, h, 0, 0, pl, pt, F(nw) / F(w), F(nh) / F(h))
        records = [rec[(n, s)] for n in range(2) for s in range(3)]
        views = cl.TileGeometry.from_records(records, [0, 3, 6], "cuda")
        dets = {key: torch.stack([p[key][n] for n in range(2) for p in parts]) for key in parts[0]}          # frame-major: view n * 3 + s
        for kw in ({}, {"method": "linear", "iou_threshold": 0.3, "class_aware": False, "max_detections": 40, "score_threshold": 0.02}):
            want = model.merge_soft(dets["bboxes"], dets["scores"], dets["labels"], views, **kw)
            got = model.detect_multiscale(frames, scales=scales, height=128, width=128, flip_test=flip_test, num_detections=50, fill=fill, **kw)
            assert set(got) == ({"bboxes", "labels", "scores", "count", "embeddings"} if tracking else {"bboxes", "labels", "scores", "count"})
            K = kw.get("max_detections", 100)
            assert tuple(got["bboxes"].shape) == (2, K, 4) and got["count"].dtype == torch.int32
            for key in ("bboxes", "labels", "scores", "count"):
                assert np.array_equal(got[key].cpu().numpy().view(np.uint8), want[key].cpu().numpy().view(np.uint8)), (flip_test, kw, key)
            count = got["count"].cpu().numpy()
            assert (count > 0).all()
            source = want["source"].cpu().numpy()
            d = {key: v.cpu().numpy() for key, v in dets.items()}
            if kw.get("method") == "linear":                                                  # no exp: these real detections against the restatement, exactly
                restated = ref.soft_merge_ref(d["bboxes"], d["scores"], d["labels"], records, [0, 3, 6], K,
                                                  **{key: v for key, v in kw.items() if key != "max_detections"})
                assert np.array_equal(restated["source"], source) and np.array_equal(restated["count"], count)
                assert np.array_equal(bits(got["scores"].cpu().numpy()), bits(restated["scores"]))
            for n, (h, w) in enumerate(sizes):                                                # the boxes lie inside each frame
                b = got["bboxes"][n].cpu().numpy()
                assert b.min() >= 0 and b[:, 0::2].max() <= w and b[:, 1::2].max() <= h and (b[count[n]:] == 0).all()
                s = got["scores"][n].cpu().numpy()
                assert (np.diff(s[:count[n]]) <= 0).all() and (s[count[n]:] == 0).all()
            if tracking:
                emb = np.zeros((2, K, d["embeddings"].shape[-1]), dtype=F)
                for n in range(2):
                    emb[n, :count[n]] = d["embeddings"][3 * n:3 * n + 3].reshape(-1, emb.shape[-1])[source[n, :count[n]]]
                assert np.array_equal(bits(got["embeddings"].cpu().numpy()), bits(emb))
            # the dict feeds the evaluator as it is
            ev = model.evaluator()
            ev.update(got, [{"boxes": np.array([[10.0, 10.0, 40.0, 30.0]]), "labels": np.array([0])}, {"boxes": np.zeros((0, 4)), "labels": np.zeros((0,), np.int64)}])
            metrics = ev.get_metrics()
            assert ev.num_images == 2 and len(metrics) == 12
