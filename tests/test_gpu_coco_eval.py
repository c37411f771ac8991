"""GPU: CocoEvaluator (cnl_coco_match_f64 / cnl_coco_accumulate_f64, csrc/coco_eval.hip) against tests/coco_eval_ref.py.

Every comparison of ranks, masks, npig, precision, recall and the twelve metrics is an EQUALITY (float64 bits): the rule is IEEE
arithmetic with contraction off, so there is no tolerance to choose.  Boxes sit on an integer grid and scores come from six values, so
IoU ties, score ties and exact threshold hits occur in every case."""
import functools
import os

import numpy as np
import pytest
import torch

import bench
import coco_eval_ref as ref
import centernet_lightning_amd as cl

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")
SCORES = np.array([0.15, 0.3, 0.3, 0.55, 0.8, 0.95], np.float32)

# name: (seed, N, K, k, ground truths per image (None: random up to g_max), g_max, scale, empty images)
CASES = {
    "small": (24, 3, 3, 8, None, 5, 1, ()),                # every size below a wave; small and medium objects
    "over64": (2, 2, 2, 130, 70, 70, 1, ()),               # two lane passes over the ground truths, over 100 detections of a class, k over a wave
    "empty": (3, 5, 3, 8, None, 5, 1, (2,)),               # one image empty on both sides
    "scaled": (4, 4, 3, 12, None, 6, 4, ()),               # boxes x 4: areas straddle 32^2 AND 96^2, every range is populated
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (boxes [N,k,4] f32 xyxy, scores, labels (some outside 0..K-1), count, per-image ground truths [(xywh f64, labels)], K)."""
    seed, N, K, k, g_fixed, g_max, scale, empty = CASES[name]
    rng = np.random.default_rng(seed)
    xy, wh = rng.integers(0, 41, (N, k, 2)), rng.integers(1, 41, (N, k, 2))
    for n in range(N):                                     # a third of the detections crowd around another one: they compete for its object
        for d in rng.choice(k, k // 3, replace=False):
            e = int(rng.integers(0, k))
            xy[n, d], wh[n, d] = np.clip(xy[n, e] + rng.integers(-2, 3, 2), 0, 40), np.clip(wh[n, e] + rng.integers(-2, 3, 2), 1, 40)
    boxes = (np.concatenate([xy, xy + wh], -1) * scale).astype(np.float32)
    # (two classes: six in seven detections are of class 0, so that a 130-slot image holds more than 100 of one class)
    scores, labels = rng.choice(SCORES, (N, k)), rng.integers(-1, K + 1, (N, k)) if K > 2 else (rng.integers(0, 7, (N, k)) == 0).astype(np.int64)
    count = rng.integers(k // 2, k + 1, N).astype(np.int32)
    count[0] = k
    gts = []
    for n in range(N):
        g = g_fixed if g_fixed is not None else int(rng.integers(1, g_max + 1))
        if n in empty:                                     # no ground truth, and no detection either: count 0, or every label dropped
            g, count[n], labels[n] = 0, 0, -1
        gxy, gwh, gl = rng.integers(0, 41, (g, 2)), rng.integers(1, 41, (g, 2)), rng.integers(0, K, g)
        for j in range(g):                                 # three in four objects sit on or near a detection and carry its label
            if rng.random() < 0.75:
                d = int(rng.integers(0, k))
                gxy[j], gwh[j] = np.clip(xy[n, d] + rng.integers(-3, 4, 2), 0, 40), np.clip(wh[n, d] + rng.integers(-3, 4, 2), 1, 40)
                gl[j] = labels[n, d] if 0 <= labels[n, d] < K else gl[j]
        if g and n == 0:
            gxy[0], gwh[0], gl[0] = xy[0, 0], wh[0, 0], min(max(labels[0, 0], 0), K - 1)            # at least one exact hit
            labels[0, 0] = gl[0]
        gts.append(((np.concatenate([gxy, gwh], -1) * scale).astype(np.float64), gl))
    return boxes, scores.astype(np.float32), labels.astype(np.int64), count, gts, K


@functools.lru_cache(maxsize=None)
def expected(name, gated=False):
    """The restatement's answer, computed once per case (gated: only the first count[n] slots of image n hold detections)."""
    boxes, scores, labels, count, gts, K = case(name)
    dets = [(boxes[n, :c], scores[n, :c], labels[n, :c]) for n, c in enumerate(count if gated else [boxes.shape[1]] * len(boxes))]
    return ref.evaluate(dets, gts, K)


def device_dict(name, images=None, gated=False):
    boxes, scores, labels, count, _, _ = case(name)
    sel = slice(None) if images is None else list(images)
    out = {"bboxes": torch.from_numpy(boxes[sel]).cuda(), "scores": torch.from_numpy(scores[sel]).cuda(), "labels": torch.from_numpy(labels[sel]).cuda()}
    if gated:
        out["count"] = torch.from_numpy(count[sel]).cuda()
    return out


def target_list(name, images=None):
    gts = case(name)[4]
    return [{"boxes": gts[n][0], "labels": gts[n][1]} for n in (range(len(gts)) if images is None else images)]


def padded_targets(name, images=None):
    gts = [case(name)[4][n] for n in (range(len(case(name)[4])) if images is None else images)]
    g_max = max([1] + [len(l) for _, l in gts])
    boxes, labels = np.full((len(gts), g_max, 4), 7.0), np.full((len(gts), g_max), 1, np.int64)      # the padding must not count
    for n, (b, l) in enumerate(gts):
        boxes[n, :len(l)], labels[n, :len(l)] = b, l
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda(), torch.tensor([len(l) for _, l in gts], dtype=torch.int32).cuda()


def same_metrics(got, want):
    assert list(got) == list(ref.METRIC_NAMES) and all(type(v) is float for v in got.values())
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}


def assert_equals_ref(ev, want):
    metrics = ev.get_metrics()
    assert ev.precision.shape == want["precision"].shape and ev.recall.shape == want["recall"].shape and ev.precision.dtype == np.float64
    bad = np.argwhere(ev.precision != want["precision"])
    assert np.array_equal(ev.precision, want["precision"]), (len(bad), bad[:5], ev.precision[tuple(bad[0])], want["precision"][tuple(bad[0])])
    assert np.array_equal(ev.recall, want["recall"]), np.argwhere(ev.recall != want["recall"])[:5]
    same_metrics(metrics, want["metrics"])
    return metrics


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_match_records_and_npig(name, gated):
    boxes, scores, labels, count, gts, K = case(name)
    N, k = scores.shape
    want = expected(name, gated)
    ev = cl.CocoEvaluator(K)
    ev.update(device_dict(name, gated=gated), target_list(name))
    st = ev.state()
    assert st["num_images"] == N and st["num_classes"] == K and tuple(st["rank"].shape) == (N * k,)
    assert np.array_equal(st["npig"].cpu().numpy(), want["npig"])
    rank, matched, ignored = (st[key].cpu().numpy().reshape(N, k) for key in ("rank", "matched", "ignored"))
    assert np.array_equal(st["score"].cpu().numpy().reshape(N, k), scores) and np.array_equal(st["label"].cpu().numpy().reshape(N, k), labels)
    for n in range(N):
        c = count[n] if gated else k
        _, _, r, m, i = want["records"][n]
        assert np.array_equal(rank[n, :c], r), (n, rank[n, :c], r)
        assert np.array_equal(matched[n, :c], m), (n, [hex(v) for v in matched[n, :c]], [hex(v) for v in m])
        assert np.array_equal(ignored[n, :c], i), (n, [hex(v) for v in ignored[n, :c]], [hex(v) for v in i])
        assert (rank[n, c:] == -1).all() and (matched[n, c:] == 0).all() and (ignored[n, c:] == 0).all()      # slots past the count
    if name == "over64":
        assert (rank == -1).any() and rank.max() == 99 and want["npig"].sum() > 64
    if name == "scaled":
        assert (want["npig"].sum(0) > 0).all()             # every area range holds ground truths


@pytest.mark.parametrize("name", list(CASES))
def test_one_update_equals_ref(name):
    ev = cl.CocoEvaluator(case(name)[5])
    ev.update(device_dict(name), target_list(name))
    metrics = assert_equals_ref(ev, expected(name))
    if name == "scaled":
        assert all(v > -1 for v in metrics.values())
    else:
        assert metrics["AP_large"] == -1.0 and metrics["mAP"] > 0       # boxes up to 40 x 40 never reach 96^2


@pytest.mark.parametrize("name", list(CASES))
def test_three_updates_reset_and_reuse(name):
    N, K = len(case(name)[0]), case(name)[5]
    ev = cl.CocoEvaluator(K, device="cuda")
    for part in np.array_split(np.arange(N), 3):           # (an empty batch among them when N < 3)
        ev.update(device_dict(name, part.tolist()), padded_targets(name, part.tolist()) if len(part) else target_list(name, []))
    assert ev.num_images == N
    assert_equals_ref(ev, expected(name))
    assert_equals_ref(ev, expected(name))                  # get_metrics changes nothing
    ev.reset()
    assert ev.num_images == 0 and ev.precision is None
    ev.update(device_dict("small"), target_list("small"))  # another epoch in the same buffers
    if K == case("small")[5]:
        assert_equals_ref(ev, expected("small"))
    ev.reset()
    ev.update(device_dict(name), target_list(name))
    assert_equals_ref(ev, expected(name))


@pytest.mark.parametrize("name", ["small", "empty", "scaled"])
def test_merge_of_two_shards_equals_one_evaluator(name):
    N, K = len(case(name)[0]), case(name)[5]
    one = cl.CocoEvaluator(K)
    one.update(device_dict(name), target_list(name))
    single = one.get_metrics()
    first, second = list(range(N // 2)), list(range(N // 2, N))
    a, b = cl.CocoEvaluator(K), cl.CocoEvaluator(K)
    a.update(device_dict(name, first), target_list(name, first))
    b.update(device_dict(name, second), target_list(name, second))
    a.merge(b.state())
    assert a.num_images == N
    same_metrics(a.get_metrics(), single)
    assert np.array_equal(a.precision, one.precision) and np.array_equal(a.recall, one.recall)
    assert_equals_ref(a, expected(name))
    sa, so = a.state(), one.state()
    for key in ("score", "label", "rank", "matched", "ignored", "npig"):
        assert torch.equal(sa[key], so[key]), key
    with pytest.raises(ValueError):
        a.merge({**b.state(), "num_classes": K + 1})


@pytest.mark.parametrize("name", ["small", "over64", "empty"])
def test_count_gate_equals_shorter_inputs(name):
    boxes, scores, labels, count, gts, K = case(name)
    gated = cl.CocoEvaluator(K)
    gated.update(device_dict(name, gated=True), target_list(name))
    assert_equals_ref(gated, expected(name, gated=True))
    # the same detections as physically shorter inputs, image by image
    short = cl.CocoEvaluator(K)
    for n, c in enumerate(count):
        c = int(c)
        if c == 0:                                         # k >= 1: an image without detections is a count of 0
            d = {"bboxes": torch.zeros((1, 1, 4)).cuda(), "scores": torch.zeros((1, 1)).cuda(), "labels": torch.zeros((1, 1), dtype=torch.int64).cuda(),
                 "count": torch.zeros((1,), dtype=torch.int32).cuda()}
        else:
            d = {"boxes": torch.from_numpy(boxes[n:n + 1, :c]).cuda(), "scores": torch.from_numpy(scores[n:n + 1, :c]).cuda(),
                 "labels": torch.from_numpy(labels[n:n + 1, :c]).cuda()}
        short.update(d, target_list(name, [n]))
    same_metrics(short.get_metrics(), gated.get_metrics())
    assert np.array_equal(short.precision, gated.precision) and np.array_equal(short.recall, gated.recall)
    # an int64 count is accepted too
    again = cl.CocoEvaluator(K)
    d = device_dict(name, gated=True)
    again.update({**d, "count": d["count"].long()}, target_list(name))
    same_metrics(again.get_metrics(), gated.get_metrics())
    assert np.array_equal(again.precision, gated.precision)


@pytest.mark.parametrize("name", ["small", "empty", "scaled"])
def test_reference_list_form_equals_device_form(name):
    boxes, scores, labels, count, gts, K = case(name)
    preds = []
    for n, c in enumerate(count):                          # per-image dicts with xywh numpy boxes, as the reference's validation_step builds them
        b = boxes[n, :c]
        preds.append({"boxes": np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], 1), "scores": scores[n, :c], "labels": labels[n, :c]})
    ev = cl.CocoEvaluator(K)
    ev.update(preds, target_list(name))
    assert_equals_ref(ev, expected(name, gated=True))
    # torch CPU tensors per image work as well
    ev.reset()
    ev.update([{key: torch.from_numpy(np.ascontiguousarray(v)) for key, v in p.items()} for p in preds],
              [{key: torch.from_numpy(np.ascontiguousarray(v)) for key, v in t.items()} for t in target_list(name)])
    assert_equals_ref(ev, expected(name, gated=True))


def test_limits_on_the_device():
    ev = cl.CocoEvaluator(2)
    k = 1024                                               # the largest supported image: the kernel's 70 KB of dynamic LDS
    rng = np.random.default_rng(5)
    xy, wh = rng.integers(0, 41, (1, k, 2)), rng.integers(1, 41, (1, k, 2))
    boxes = np.concatenate([xy, xy + wh], -1).astype(np.float32)
    scores, labels = rng.choice(SCORES, (1, k)).astype(np.float32), rng.integers(0, 2, (1, k)).astype(np.int64)
    g = 1024
    gts = (np.concatenate([rng.integers(0, 41, (g, 2)), rng.integers(1, 41, (g, 2))], -1).astype(np.float64), rng.integers(0, 2, g))
    # (the restatement walks 1024 x 1024 pairs 40 times in Python: compare the cheap parts only — ranks and npig — and that it runs)
    ev.update({"bboxes": torch.from_numpy(boxes).cuda(), "scores": torch.from_numpy(scores).cuda(), "labels": torch.from_numpy(labels).cuda()},
              [{"boxes": gts[0], "labels": gts[1]}])
    st = ev.state()
    rank = st["rank"].cpu().numpy()
    for c in range(2):
        mine = np.flatnonzero(labels[0] == c)
        order = mine[np.argsort(-scores[0][mine], kind="stable")]
        assert np.array_equal(rank[order[:100]], np.arange(100)) and (rank[order[100:]] == -1).all()
    area = gts[0][:, 2] * gts[0][:, 3]
    want = [[int(((gts[1] == c) & (area >= lo) & (area <= hi)).sum()) for lo, hi in ref.AREA_RANGES] for c in range(2)]
    assert st["npig"].cpu().tolist() == want
    metrics = ev.get_metrics()
    assert 0 < metrics["mAP"] < 1 and metrics["AP_large"] == -1.0
    with pytest.raises(ValueError):
        ev.update({"bboxes": torch.zeros((1, 1025, 4)).cuda(), "scores": torch.zeros((1, 1025)).cuda(),
                   "labels": torch.zeros((1, 1025), dtype=torch.int64).cuda()}, [{"boxes": gts[0], "labels": gts[1]}])


def test_end_to_end_model_to_metrics():
    """A seeded tiny model on 4 images of 128 x 128, the targets made from its own detections: gather_detection2d's dict goes straight
    into update, every detection finds its own box at IoU exactly 1, so AP50 is 1 up to np.spacing(1) in the precisions."""
    torch.manual_seed(0)
    model = bench.synthetic_weights_(cl.build_centernet(os.path.join(CONFIGS, bench.CONFIGS["fpn"]))).cuda()
    x = torch.rand((4, 3, 128, 128), generator=torch.Generator().manual_seed(11)).cuda()
    dets = model.gather_detection2d(model(x), num_detections=16)
    b = dets["bboxes"].cpu().numpy()
    assert b.dtype == np.float32 and ((b[..., 2] - b[..., 0]) > 0).all() and ((b[..., 3] - b[..., 1]) > 0).all()
    wh = np.stack([b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1)                      # fp32, as the rule forms them
    targets = [{"boxes": np.concatenate([b[n, :, :2], wh[n]], 1).astype(np.float64), "labels": dets["labels"][n].cpu().numpy()} for n in range(4)]
    ev = model.evaluator()
    ev.update(dets, targets)
    metrics = ev.get_metrics()
    assert abs(metrics["AP50"] - 1) < 1e-12 and abs(metrics["mAP"] - 1) < 1e-12 and abs(metrics["mAR"] - 1) < 1e-12
    want = ref.evaluate([(b[n], dets["scores"][n].cpu().numpy(), dets["labels"][n].cpu().numpy()) for n in range(4)],
                        [(t["boxes"], t["labels"]) for t in targets], model.num_classes)
    assert np.array_equal(ev.precision, want["precision"]) and np.array_equal(ev.recall, want["recall"])
    same_metrics(metrics, want["metrics"])
