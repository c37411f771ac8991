"""No GPU: the COCO evaluation's numpy restatement (tests/coco_eval_ref.py) on hand-derived cases — pycocotools is not available, so
these pin the restatement itself —, the two entry points' C-ABI declarations and argument checks, the Python surface's refusals, and
the equivalence of the kernel's wave-form choice with the sequential rule of the statement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import coco_eval_ref as ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, coco_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnl_coco_match_f64", "cnl_coco_accumulate_f64")
TOL = 1e-12


def image(dets_xywh, scores, labels, gts_xywh, gt_labels):
    """One image in the restatement's form from xywh detections on a grid where x + w is exact in fp32."""
    return ((ref.xywh_to_xyxy32(dets_xywh), np.asarray(scores, np.float32), np.asarray(labels, np.int64)),
            (np.asarray(gts_xywh, np.float64).reshape(-1, 4), np.asarray(gt_labels, np.int64)))


def evaluate(images, num_classes=1):
    return ref.evaluate([d for d, _ in images], [g for _, g in images], num_classes)


def bits(mask, a):
    """The ten threshold bits of area range a."""
    return [(int(mask) >> (a * 10 + t)) & 1 for t in range(10)]


# ----------------------------------------------------------------------------- the restated rule on hand-derived cases
def test_parameters():
    assert ref.IOU_THRS[0] == 0.5 and ref.IOU_THRS[5] == 0.75 and ref.IOU_THRS[-1] == 0.95 and len(ref.IOU_THRS) == 10
    assert len(ref.REC_THRS) == 101 and ref.REC_THRS[50] == 0.5 and ref.REC_THRS[-1] == 1.0
    # the doubles csrc/coco_eval.hip carries as literals / forms as i * 0.01
    assert ref.IOU_THRS.tolist() == [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.8999999999999999, 0.95]
    assert all(ref.REC_THRS[i] == (1.0 if i == 100 else i * 0.01) for i in range(101))
    assert ref.METRIC_NAMES == cl.CocoEvaluator.metric_names == coco_eval.METRIC_NAMES and len(ref.METRIC_NAMES) == 12
    assert np.spacing(1) == 2.0 ** -52


def test_worked_example():
    out = evaluate([image([[0, 0, 10, 10], [50, 50, 10, 10], [20, 0, 10, 6.2]], [0.9, 0.8, 0.7], [0, 0, 0],
                          [[0, 0, 10, 10], [20, 0, 10, 10]], [0, 0])])
    rank, matched, ignored = out["records"][0][2:]
    assert rank.tolist() == [0, 1, 2]
    assert bits(matched[0], 0) == [1] * 10 and bits(matched[1], 0) == [0] * 10 and bits(matched[2], 0) == [1, 1, 1] + [0] * 7      # IoU 0.62
    m = out["metrics"]
    ap50, ap75 = (51 + 50 * 2 / 3) / 101, 51 / 101
    assert abs(m["AP50"] - ap50) < TOL and abs(m["AP75"] - ap75) < TOL
    assert abs(m["mAP"] - (3 * ap50 + 7 * 51 / 101) / 10) < TOL and abs(m["AP_small"] - m["mAP"]) < TOL
    assert m["AP_medium"] == -1 and m["AP_large"] == -1 and m["AR_medium"] == -1 and m["AR_large"] == -1
    assert abs(m["AR1"] - 0.5) < TOL
    for name in ("AR10", "mAR", "AR_small"):
        assert abs(m[name] - 0.65) < TOL, name
    assert m["AP50"] < ap50                       # np.spacing(1) keeps the precisions a hair under the fractions
    assert list(m) == list(ref.METRIC_NAMES)
    assert out["npig"].tolist() == [[2, 2, 0, 0]]


def test_all_detections_perfect():
    gts = [[0, 0, 10, 10], [20, 0, 40, 40], [100, 100, 100, 100]]            # small, medium, large
    out = evaluate([image(gts, [0.9, 0.8, 0.7], [0, 1, 0], gts, [0, 1, 0])], num_classes=2)
    for name, v in out["metrics"].items():
        assert abs(v - (0.75 if name == "AR1" else 1.0)) < TOL, (name, v)     # AR1: category 0 has two objects and one detection allowed: (1/2 + 1) / 2
    assert out["npig"].tolist() == [[2, 1, 0, 1], [1, 0, 1, 0]]


def test_no_detections_at_all():
    out = evaluate([image(np.zeros((0, 4)), [], [], [[0, 0, 10, 10]], [0])])
    m = out["metrics"]
    for name in ("mAP", "AP50", "AP75", "AP_small", "AR1", "AR10", "mAR", "AR_small"):
        assert m[name] == 0.0, name
    for name in ("AP_medium", "AP_large", "AR_medium", "AR_large"):
        assert m[name] == -1.0, name
    assert (out["precision"][:, :, 0, 0, :] == 0).all() and (out["precision"][:, :, 0, 2, :] == -1).all()


def test_image_with_detections_and_no_ground_truth():
    # image 0: one object found at 0.9; image 1: no object, one detection at 0.95 -> [fp, tp]: precision 1/2 at every recall
    out = evaluate([image([[0, 0, 10, 10]], [0.9], [0], [[0, 0, 10, 10]], [0]), image([[5, 5, 10, 10]], [0.95], [0], np.zeros((0, 4)), [])])
    m = out["metrics"]
    assert abs(m["AP50"] - 0.5) < TOL and abs(m["mAP"] - 0.5) < TOL and abs(m["mAR"] - 1.0) < TOL
    assert out["records"][1][2].tolist() == [0] and out["records"][1][3].tolist() == [0]
    # a category nobody annotated stays -1 whatever is detected
    out = evaluate([image([[0, 0, 10, 10]], [0.9], [1], [[0, 0, 10, 10]], [0])], num_classes=2)
    assert (out["precision"][:, :, 1] == -1).all() and (out["recall"][:, 1] == -1).all() and out["metrics"]["AP50"] == 0.0


def test_iou_exactly_at_a_threshold_matches():
    assert ref.iou_xywh((0, 0, 10, 10), (0, 0, 10, 5)) == 0.5
    out = evaluate([image([[0, 0, 10, 5]], [0.9], [0], [[0, 0, 10, 10]], [0])])
    assert bits(out["records"][0][3][0], 0) == [1] + [0] * 9
    m = out["metrics"]
    assert abs(m["AP50"] - 1) < TOL and m["AP75"] == 0.0 and abs(m["mAP"] - 0.1) < TOL and abs(m["mAR"] - 0.1) < TOL


def test_two_identical_ground_truths_the_later_is_taken_first():
    trace = {}
    d, g = image([[0, 0, 10, 10], [0, 0, 10, 10]], [0.9, 0.8], [0, 0], [[0, 0, 10, 10], [0, 0, 10, 10]], [0, 0])
    rank, matched, ignored, npig = ref.match_image(*d, *g, 1, trace=trace)
    assert trace[0, 0, 0] == 1 and trace[0, 0, 1] == 0 and trace[0, 9, 0] == 1          # equal IoU: `iou < best` does not skip, the later wins
    assert bits(matched[0], 0) == [1] * 10 and bits(matched[1], 0) == [1] * 10 and npig.tolist() == [[2, 2, 0, 0]]


def test_equal_scores_go_by_arrival():
    # both detections fit the one object; the same score: the first to arrive is rank 0 and takes it
    d, g = image([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]], [0.5, 0.7, 0.5], [0, 0, 0], [[0, 0, 10, 10]], [0])
    rank, matched, _, _ = ref.match_image(*d, *g, 1)
    assert rank.tolist() == [1, 0, 2] and [bits(m, 0)[0] for m in matched] == [0, 1, 0]
    d, g = image([[0, 0, 10, 10], [0, 0, 10, 10]], [0.5, 0.5], [0, 0], [[0, 0, 10, 10]], [0])
    rank, matched, _, _ = ref.match_image(*d, *g, 1)
    assert rank.tolist() == [0, 1] and [bits(m, 0)[0] for m in matched] == [1, 0]
    # across images the stable sort keeps image order: [tp (image 0), fp (image 1)] -> AP 1, not 1/2
    out = evaluate([image([[0, 0, 10, 10]], [0.5], [0], [[0, 0, 10, 10]], [0]), image([[0, 0, 10, 10]], [0.5], [0], np.zeros((0, 4)), [])])
    assert abs(out["metrics"]["AP50"] - 1) < TOL
    out = evaluate([image([[0, 0, 10, 10]], [0.5], [0], np.zeros((0, 4)), []), image([[0, 0, 10, 10]], [0.5], [0], [[0, 0, 10, 10]], [0])])
    assert abs(out["metrics"]["AP50"] - 0.5) < TOL


def test_area_exactly_1024_is_small_and_medium():
    assert not ref.out_of_range(1024.0, 1) and not ref.out_of_range(1024.0, 2) and ref.out_of_range(1024.0, 3)
    assert not ref.out_of_range(9216.0, 2) and not ref.out_of_range(9216.0, 3) and ref.out_of_range(9216.0, 1)
    out = evaluate([image([[0, 0, 32, 32]], [0.9], [0], [[0, 0, 32, 32]], [0])])
    assert out["npig"].tolist() == [[1, 1, 1, 0]]
    m = out["metrics"]
    assert abs(m["AP_small"] - 1) < TOL and abs(m["AP_medium"] - 1) < TOL and m["AP_large"] == -1
    ignored = out["records"][0][4][0]
    assert bits(ignored, 3) == [1] * 10 and bits(ignored, 1) == [0] * 10 and bits(ignored, 2) == [0] * 10      # `large`: matched to an ignored object


def test_in_range_ground_truth_wins_over_a_better_out_of_range_one():
    # detection 40 x 30 (area 1200); object 0: 40 x 40 (1600, medium), IoU 0.75; object 1: 40 x 25 (1000, small), IoU 0.8333
    trace = {}
    d, g = image([[0, 0, 40, 30]], [0.9], [0], [[0, 0, 40, 40], [0, 0, 40, 25]], [0, 0])
    assert ref.iou_xywh((0, 0, 40, 30), (0, 0, 40, 40)) == 0.75 and abs(ref.iou_xywh((0, 0, 40, 30), (0, 0, 40, 25)) - 5 / 6) < 1e-15
    rank, matched, ignored, npig = ref.match_image(*d, *g, 1, trace=trace)
    assert npig.tolist() == [[2, 1, 1, 0]]
    assert trace[0, 0, 0] == 1                     # all: both in range, the larger IoU
    assert trace[2, 0, 0] == 0                     # medium: object 0 is in range and wins at the lower IoU
    assert trace[1, 0, 0] == 1 and trace[1, 6, 0] == 1 and (1, 7, 0) not in trace          # small: object 1, up to t = 0.8
    assert trace[2, 5, 0] == 0 and trace[2, 6, 0] == 1          # medium at t = 0.8: only the ignored object reaches it ...
    assert bits(matched[0], 2) == [1] * 7 + [0] * 3
    assert bits(ignored[0], 2) == [0] * 6 + [1] + [0] * 3        # ... so the detection is ignored there; above it is unmatched, and its own area (1200) is medium
    assert bits(matched[0], 1) == [1] * 7 + [0] * 3 and bits(ignored[0], 1) == [0] * 7 + [1] * 3      # small: unmatched above 0.8 and out of range itself


def test_130_detections_of_one_class_keep_100():
    n = 130
    boxes = [[i, 0, 5, 5] for i in range(n)]
    scores = np.linspace(0.1, 0.9, n).astype(np.float32)           # ascending: the LAST slots rank first
    d, g = image(boxes, scores, [0] * n, [[0, 0, 5, 5]], [0])
    rank, matched, ignored, _ = ref.match_image(*d, *g, 1)
    assert rank[-1] == 0 and rank[30] == 99 and (rank[:30] == -1).all() and sorted(rank[30:].tolist()) == list(range(100))
    assert (matched[:30] == 0).all() and (ignored[:30] == 0).all()
    # the object sits under slot 0, which was dropped: nothing finds it
    assert bits(matched[0], 0) == [0] * 10 and evaluate([(d, g)])["metrics"]["mAR"] < 1
    # labels outside 0..K-1 are dropped on both sides
    d, g = image([[0, 0, 5, 5], [0, 0, 5, 5]], [0.9, 0.8], [3, -1], [[0, 0, 5, 5]], [7])
    rank, matched, ignored, npig = ref.match_image(*d, *g, 3)
    assert rank.tolist() == [-1, -1] and not npig.any()


# ----------------------------------------------------------------------------- the wave form of the choice
def wave_match_image(boxes_xyxy, scores, labels, gt_xywh, gt_labels, num_classes, lanes=4):
    """The kernel's form of the match, sequentially: ranks by counting the detections ahead; per (a, t) and detection ONE maximum over
    the key (not ignored, IoU) of the eligible ground truths, chunk by chunk of `lanes`, the last among equals winning."""
    D = ref.detections_xywh(boxes_xyxy)
    scores, labels = np.asarray(scores, np.float32), np.asarray(labels, np.int64)
    G = [tuple(float(v) for v in g) for g in np.asarray(gt_xywh, np.float64).reshape(-1, 4)]
    n = len(D)
    rank = np.full(n, -1, np.int32)
    matched, ignored = np.zeros(n, np.int64), np.zeros(n, np.int64)
    order = {}
    for d in range(n):
        if not 0 <= labels[d] < num_classes:
            continue
        valid = [e for e in range(n) if 0 <= labels[e] < num_classes]
        before = sum(1 for e in valid if labels[e] < labels[d])
        ahead = sum(1 for e in valid if labels[e] == labels[d] and (scores[e] > scores[d] or (scores[e] == scores[d] and e < d)))
        if ahead < 100:
            rank[d] = ahead
            order[before + ahead] = d
    for a in range(4):
        taken = [0] * len(G)
        for p in sorted(order):
            d = order[p]
            best_key, best_g = [(0, 0.0)] * 10, [None] * 10
            for g0 in range(0, len(G), lanes):
                chunk = [g for g in range(g0, min(g0 + lanes, len(G))) if gt_labels[g] == labels[d]]
                iou = {g: ref.iou_xywh(D[d], G[g]) for g in chunk}
                for t in range(10):
                    thr = min(float(ref.IOU_THRS[t]), 1 - 1e-10)
                    elig = [g for g in chunk if iou[g] >= thr and not (taken[g] >> t) & 1]
                    if not elig:
                        continue
                    key = {g: (0 if ref.out_of_range(G[g][2] * G[g][3], a) else 1, iou[g]) for g in elig}
                    kmax = max(key.values())
                    if kmax >= best_key[t]:
                        best_key[t], best_g[t] = kmax, max(g for g in elig if key[g] == kmax)
            for t in range(10):
                bit = 1 << (a * 10 + t)
                if best_g[t] is not None:
                    taken[best_g[t]] |= 1 << t
                    matched[d] |= bit
                    if best_key[t][0] == 0:
                        ignored[d] |= bit
                elif ref.out_of_range(D[d][2] * D[d][3], a):
                    ignored[d] |= bit
    return rank, matched, ignored


def test_wave_form_equals_the_sequential_rule():
    rng = np.random.default_rng(7)
    score_set = np.array([0.2, 0.4, 0.4, 0.6, 0.8, 0.9], np.float32)
    ties = 0
    for case in range(3000):
        n, g, scale = int(rng.integers(0, 7)), int(rng.integers(0, 7)), int(rng.choice([1, 1, 4]))
        xy, wh = rng.integers(0, 5, (n, 2)) * 8 * scale, rng.integers(1, 6, (n, 2)) * 8 * scale          # a coarse grid: IoU ties and threshold hits occur
        gxy, gwh = rng.integers(0, 5, (g, 2)) * 8 * scale, rng.integers(1, 6, (g, 2)) * 8 * scale
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        gts = np.concatenate([gxy, gwh], 1).astype(np.float64)
        scores, labels, gl = rng.choice(score_set, n), rng.integers(-1, 3, n), rng.integers(0, 2, g)
        want = ref.match_image(boxes, scores, labels, gts, gl, 2)
        got = wave_match_image(boxes, scores, labels, gts, gl, 2, lanes=int(rng.choice([2, 4, 64])))
        for w, x, name in zip(want, got, ("rank", "matched", "ignored")):
            assert np.array_equal(w, x), (case, name, boxes, scores, labels, gts, gl)
        ious = [ref.iou_xywh(d, tuple(b)) for d in ref.detections_xywh(boxes) for b in gts]
        ties += len(ious) != len(set(ious)) or any(v in ref.IOU_THRS for v in ious)
    assert ties > 300          # the cases do exercise equal IoUs and exact threshold hits


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/centernet_gfx950.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # entry points only: no ABI bump
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
        assert set(ENTRY_POINTS) <= defined


def test_entry_points_validate_arguments_without_a_device():
    lib = _lib.load()
    E = _lib.CNL_E_BAD_ARG
    fake = 0x10000          # never dereferenced: every call below fails validation first

    def match(boxes=fake, scores=fake, labels=fake, count=None, gb=fake, gl=fake, gc=fake, N=2, k=100, Gmax=8, K=80, r=fake, m=fake, i=fake, npig=fake):
        return lib.cnl_coco_match_f64(boxes, scores, labels, count, gb, gl, gc, N, k, Gmax, K, r, m, i, npig, None)

    for name in ("boxes", "scores", "labels", "gb", "gl", "gc", "r", "m", "i", "npig"):
        assert match(**{name: None}) == E and "null" in _lib.last_error(), name
    assert match(N=-1) == E and "N = -1" in _lib.last_error()
    assert match(k=0) == E and match(k=1025) == E and "k = 1025" in _lib.last_error()
    assert match(Gmax=0) == E and match(Gmax=1025) == E and "Gmax = 1025" in _lib.last_error()
    assert match(K=0) == E and "num_classes" in _lib.last_error()
    assert match(boxes=fake + 4) == E and match(gb=fake + 4) == E and "aligned" in _lib.last_error()
    assert match(N=0, boxes=None, scores=None, labels=None, gb=None, gl=None, gc=None, r=None, m=None, i=None, npig=None) == 0      # an empty batch is a no-op

    def accumulate(rank=fake, m=fake, i=fake, first=fake, npig=fake, total=10, K=80, pr=fake, rc=fake):
        return lib.cnl_coco_accumulate_f64(rank, m, i, first, npig, total, K, pr, rc, None)

    for name in ("rank", "m", "i", "first", "npig", "pr", "rc"):
        assert accumulate(**{name: None}) == E and "null" in _lib.last_error(), name
    assert accumulate(total=-1) == E and accumulate(total=1 << 31) == E and "total" in _lib.last_error()
    assert accumulate(K=0) == E and accumulate(pr=fake + 4) == E and accumulate(rank=fake + 2) == E


# ----------------------------------------------------------------------------- Python surface
def test_python_surface_and_refusals():
    assert "CocoEvaluator" in cl.__all__ and cl.CocoEvaluator is coco_eval.CocoEvaluator
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    ev = model.evaluator()
    assert isinstance(ev, cl.CocoEvaluator) and ev.num_classes == model.num_classes
    for name in ("update", "get_metrics", "reset", "state", "merge"):
        assert callable(getattr(ev, name))
    for bad in (0, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError):
            cl.CocoEvaluator(bad)
    with pytest.raises(RuntimeError):
        cl.CocoEvaluator(3, device="cpu")
    ev = cl.CocoEvaluator(3)
    with pytest.raises(RuntimeError):
        ev.get_metrics()                                   # nothing evaluated yet
    with pytest.raises(RuntimeError):
        ev.state()
    N, k = 2, 5
    good = {"bboxes": torch.zeros((N, k, 4)), "scores": torch.zeros((N, k)), "labels": torch.zeros((N, k), dtype=torch.int64)}
    targets = [{"boxes": np.zeros((1, 4)), "labels": np.zeros((1,), np.int64)}] * N
    with pytest.raises(RuntimeError):
        ev.update(good, targets)                           # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ev.update({"boxes": good["bboxes"], "scores": good["scores"], "labels": good["labels"]}, targets)      # the other spelling of the key
    for key, value in (("bboxes", torch.zeros((N, k, 4), dtype=torch.float64)), ("bboxes", torch.zeros((N, k, 5))), ("bboxes", torch.zeros((N * k, 4))),
                       ("bboxes", np.zeros((N, k, 4), np.float32)), ("scores", torch.zeros((N, k + 1))), ("scores", torch.zeros((N, k), dtype=torch.float16)),
                       ("labels", torch.zeros((N, k), dtype=torch.int32)), ("labels", torch.zeros((N, k, 1), dtype=torch.int64)),
                       ("count", torch.zeros((N + 1,), dtype=torch.int32)), ("count", torch.zeros((N,), dtype=torch.float32)), ("count", [k] * N)):
        with pytest.raises(ValueError):
            ev.update({**good, key: value}, targets)
    with pytest.raises(ValueError):
        ev.update({"scores": good["scores"], "labels": good["labels"]}, targets)
    with pytest.raises(ValueError):
        ev.update("detections", targets)
    big = {"bboxes": torch.zeros((1, 1025, 4)), "scores": torch.zeros((1, 1025)), "labels": torch.zeros((1, 1025), dtype=torch.int64)}
    with pytest.raises(ValueError, match="1025"):
        ev.update(big, targets[:1])                        # k over 1024
    # the reference's list form: what can be refused before anything is uploaded
    det = {"boxes": np.zeros((2, 4), np.float32), "scores": np.zeros((2,), np.float32), "labels": np.zeros((2,), np.int64)}
    with pytest.raises(ValueError, match="2 images"):
        ev.update([det, det], targets + targets[:1])       # mismatched list lengths
    with pytest.raises(ValueError, match="1025"):
        ev.update([det], [{"boxes": np.zeros((1025, 4)), "labels": np.zeros((1025,), np.int64)}])      # Gmax over 1024
    with pytest.raises(ValueError, match="1025"):
        ev.update([{"boxes": np.zeros((1025, 4)), "scores": np.zeros((1025,)), "labels": np.zeros((1025,), np.int64)}], targets[:1])
    for bad in ({"boxes": np.zeros((2, 3)), "scores": det["scores"], "labels": det["labels"]}, {"boxes": det["boxes"], "labels": det["labels"]},
                {"boxes": det["boxes"], "scores": np.zeros((3,)), "labels": det["labels"]}, "image"):
        with pytest.raises(ValueError):
            ev.update([bad], targets[:1])
    for bad in ({"boxes": np.zeros((2, 4)), "labels": np.zeros((3,), np.int64)}, {"labels": np.zeros((1,), np.int64)}, None):
        with pytest.raises(ValueError):
            ev.update([det], [bad])
    with pytest.raises(ValueError):
        ev.update([det], 5)
    # padded device targets: dtypes and shapes first, then the device
    tb, tl, tc = torch.zeros((N, 3, 4), dtype=torch.float64), torch.zeros((N, 3), dtype=torch.int64), torch.zeros((N,), dtype=torch.int32)
    for bad in ((tb.float(), tl, tc), (tb, tl.int(), tc), (tb, tl, tc.long()), (tb[:, :, :3], tl, tc), (tb, tl[:1], tc), (tb, tl, tc[:1]),
                {"boxes": tb, "labels": tl}, (torch.zeros((N, 1025, 4), dtype=torch.float64), torch.zeros((N, 1025), dtype=torch.int64), tc)):
        with pytest.raises(ValueError):
            ev.update([det, det], bad)
    with pytest.raises(RuntimeError):
        ev.update([det, det], (tb, tl, tc))
    with pytest.raises(ValueError):
        ev.merge({"score": torch.zeros(3)})
    assert ev.num_images == 0                              # nothing above left a trace


def test_summarize_matches_the_restatement():
    rng = np.random.default_rng(3)
    precision, recall = rng.random((10, 101, 5, 4, 3)), rng.random((10, 5, 4, 3))
    precision[:, :, 2], recall[:, 2] = -1, -1
    precision[:, :, :, 3], recall[:, :, 3] = -1, -1
    got, want = coco_eval.summarize(precision, recall), ref.summarize(precision, recall)
    assert list(got) == list(ref.METRIC_NAMES) and got == want and got["AP_large"] == -1.0 and all(isinstance(v, float) for v in got.values())
