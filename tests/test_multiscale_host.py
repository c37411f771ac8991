"""No GPU: the multi-scale test's host side — the soft merge's C-ABI declarations and argument checks, multiscale_sizes, the refusals of
merge_soft and detect_multiscale, and the rule itself on its numpy restatement (tests/soft_nms_ref.py): hand-made cases, the proof that
the one-loop form the kernel runs computes the two-step rule of the original CenterNet, and the margin every gaussian comparison on the
GPU rests on."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import soft_nms_ref as ref
import tiled_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnl_merge_soft_workspace_bytes", "cnl_merge_soft_f32")
F = np.float32
D = np.float64
METHODS = ("hard", "linear", "gaussian")


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in include/centernet_gfx950.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # entry points only: no ABI bump
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        assert set(ENTRY_POINTS) <= {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def workspace_formula(N, V, k, cap, with_matrix):
    """The carve-up of csrc/tile_merge.hip as the hard merge shipped it: head, keys, box, label, source, score[, the bit matrix]."""
    a = lambda v: (v + 255) & ~255
    T = V * k
    total = a(N * 16) + a(2 * T * 8) + a(T * 16) + 3 * a(T * 4)
    return total + (a(min(T, N * cap) * ((cap + 63) // 64) * 8) if with_matrix else 0)


def test_the_hard_merge_keeps_its_workspace_and_the_soft_one_has_no_matrix():
    lib = _lib.load()
    assert lib.cnl_merge_tiles_workspace_bytes(1, 5, 100, 4096) == 278784                     # the shipped value
    for (N, V, k, cap) in [(1, 5, 100, 4096), (1, 16, 100, 4096), (32, 512, 100, 4096), (3, 7, 33, 100), (2, 0, 1, 16384), (32, 160, 100, 1)]:
        assert lib.cnl_merge_tiles_workspace_bytes(N, V, k, cap) == workspace_formula(N, V, k, cap, True), (N, V, k, cap)
        if cap <= 4096:
            soft = lib.cnl_merge_soft_workspace_bytes(N, V, k, cap)
            assert soft == workspace_formula(N, V, k, cap, False) and 0 < soft <= lib.cnl_merge_tiles_workspace_bytes(N, V, k, cap)
    assert lib.cnl_merge_soft_workspace_bytes(1, 5, 100, 4097) == 0 and lib.cnl_merge_soft_workspace_bytes(1, 5, 100, 0) == 0
    assert lib.cnl_merge_soft_workspace_bytes(-1, 5, 100, 4096) == 0 and lib.cnl_merge_soft_workspace_bytes(1, 5, 0, 4096) == 0


def test_soft_merge_validates_arguments_without_a_device():
    lib = _lib.load()
    E = _lib.CNL_E_BAD_ARG
    fake = 0x10000          # never dereferenced: every call below fails validation first

    def call(boxes=fake, scores=fake, labels=fake, views=fake, ffv=fake, N=1, V=5, k=100, K_out=100, cap=4096, st=0.001, method=2, sigma=0.5, t=0.5,
             ca=1, ob=fake, os_=fake, ol=fake, osrc=fake, oc=fake, ws=fake, ws_bytes=1 << 40):
        return lib.cnl_merge_soft_f32(boxes, scores, labels, views, ffv, N, V, k, K_out, cap, st, method, sigma, t, ca, ob, os_, ol, osrc, oc, ws, ws_bytes,
                                      None)

    for name in ("boxes", "scores", "labels", "views", "ffv", "ob", "os_", "ol", "osrc", "oc"):
        assert call(**{name: None}) == E and "null" in _lib.last_error(), name
    assert call(N=-1) == E and call(V=-1) == E and call(k=0) == E and call(K_out=0) == E
    assert call(cap=0) == E and call(cap=4097) == E and "max_candidates = 4097 outside 1..4096" in _lib.last_error()
    assert call(method=3) == E and call(method=-1) == E and "method" in _lib.last_error()
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert call(sigma=sigma) == E and "sigma" in _lib.last_error(), sigma
        assert call(sigma=sigma, method=0) == E                                             # whatever the method
    assert call(st=float("nan")) == E and call(t=float("nan")) == E and "NaN" in _lib.last_error()
    assert call(boxes=fake + 4) == E and "aligned" in _lib.last_error()
    assert call(ws=None) == _lib.CNL_E_WORKSPACE and call(ws=fake + 16) == _lib.CNL_E_WORKSPACE and call(ws_bytes=16) == _lib.CNL_E_WORKSPACE
    assert call(N=0, boxes=None, scores=None, labels=None, views=None, ffv=None, ob=None, os_=None, ol=None, osrc=None, oc=None, ws=None, ws_bytes=0) == 0


# ----------------------------------------------------------------------------- the canvases
def test_multiscale_sizes():
    assert cl.multiscale_sizes(512, 512, (0.5, 0.75, 1.0, 1.25, 1.5)) == [(s, s) for s in (256, 384, 512, 640, 768)]
    assert cl.multiscale_sizes(512, 512, [1.5, 0.5]) == [(768, 768), (256, 256)]              # the order given
    assert cl.multiscale_sizes(512, 512, [0.001]) == [(32, 32)] and cl.multiscale_sizes(512, 512, (1,)) == [(512, 512)]
    assert cl.multiscale_sizes(608, 1088, (0.5, 1.0)) == [(320, 544), (608, 1088)]            # 9.5 + 0.5 -> 10 x 32: halves go up
    assert cl.multiscale_sizes(480, 640, (0.55,)) == [(256, 352)]                             # 8.25 -> 8, 11.0 -> 11
    assert len(cl.multiscale_sizes(512, 512, [0.25 * i for i in range(1, 9)])) == 8
    for bad in ([], (), [0.25 * i for i in range(1, 10)], (1.0, 1.0), (1.0, 1.01), (0.001, 0.002), (float("nan"),), (float("inf"),), (0.0,), (-1.0,),
                ("1",), (True,), (None,), 1.0, "1.0", None):
        with pytest.raises(ValueError):
            cl.multiscale_sizes(512, 512, bad)
    for h, w in ((0, 512), (512, -1), (512.0, 512), (True, 512)):
        with pytest.raises(ValueError):
            cl.multiscale_sizes(h, w, (1.0,))


# ----------------------------------------------------------------------------- the Python surface
def model():
    return cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))


BAD_VALUES = [{"method": "soft"}, {"method": 2}, {"method": None}, {"sigma": 0.0}, {"sigma": -0.5}, {"sigma": float("nan")}, {"sigma": float("inf")},
              {"sigma": "0.5"}, {"sigma": True}, {"iou_threshold": float("nan")}, {"iou_threshold": None}, {"score_threshold": float("nan")},
              {"score_threshold": "0"}, {"max_detections": 0}, {"max_detections": 2.0}, {"max_detections": True}, {"max_candidates": 0},
              {"max_candidates": 4097}, {"max_candidates": 16384}, {"max_candidates": 100.0}]


def test_merge_soft_rejects_bad_arguments_before_anything_else():
    m = model()
    for name in ("merge_soft", "detect_multiscale"):
        assert callable(getattr(m, name))
    for name in ("merge_soft", "multiscale_sizes"):
        assert hasattr(cl, name) and name in cl.__all__
    b, s, l = torch.zeros((2, 4, 4)), torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int64)
    for entry in (cl.merge_soft, m.merge_soft):
        for kw in BAD_VALUES:
            with pytest.raises(ValueError):
                entry(b, s, l, None, **kw)                                                    # a bad value wins over the CPU tensors
        for (bb, ss, ll) in [(b.double(), s, l), (b, s.half(), l), (b, s, l.int()), (b[0], s, l), (torch.zeros((2, 4, 5)), s, l), (b, s[:, :3], l),
                             (b, s, l[:1]), (b.numpy(), s, l), (b, None, l)]:
            with pytest.raises(ValueError):
                entry(bb, ss, ll, None)
        with pytest.raises(RuntimeError):
            entry(b, s, l, None)                                                              # well-formed, but on the CPU: no fallback


def test_detect_multiscale_rejects_bad_arguments_before_any_launch():
    m = model()
    frame = torch.zeros((40, 60, 3), dtype=torch.uint8)
    for kw in BAD_VALUES + [{"scales": ()}, {"scales": (1.0, 1.0)}, {"scales": (float("nan"),)}, {"scales": tuple(0.25 * i for i in range(1, 10))},
                            {"height": 0}, {"width": 100.0}]:
        with pytest.raises(ValueError):
            m.detect_multiscale([frame], **kw)                                                # (CPU frames: a RuntimeError if it got that far)
    with pytest.raises(RuntimeError):
        m.detect_multiscale([frame], scales=(0.5, 1.0), height=64, width=64)                  # no CPU fallback
    with pytest.raises(ValueError):
        m.detect_multiscale([], scales=(1.0,))


# ----------------------------------------------------------------------------- the restated rule on hand-made cases
def merge1(boxes, scores, labels, K_out=5, **kw):
    boxes = np.asarray(boxes, dtype=F).reshape(1, -1, 4)
    return ref.soft_merge_ref(boxes, np.asarray(scores, dtype=F).reshape(1, -1), np.asarray(labels).reshape(1, -1), [ref.ONE_VIEW], [0, 1], K_out,
                              **dict({"score_threshold": 0.05}, **kw))


PAIR = [[0, 0, 100, 100], [25, 0, 125, 100]]            # inter 7500, union 12500: IoU 0.6


def test_ref_the_second_of_two_overlapping_objects_survives_with_a_decayed_score():
    hard = merge1(PAIR, [0.8, 0.9], [1, 1], method="hard")
    assert hard["count"][0] == 1 and hard["source"][0].tolist() == [1, -1, -1, -1, -1] and hard["scores"][0, 0] == F(0.9)
    g = merge1(PAIR, [0.8, 0.9], [1, 1], method="gaussian", sigma=0.5)
    assert g["count"][0] == 2 and g["source"][0].tolist() == [1, 0, -1, -1, -1]
    assert g["scores64"][0, 0] == D(F(0.9)) and g["scores64"][0, 1] == D(F(0.8)) * np.exp(-(D(0.6) * D(0.6)) / D(0.5))
    assert g["scores"][0, 1] == F(g["scores64"][0, 1]) and abs(g["scores"][0, 1] - 0.8 * np.exp(-0.72)) < 1e-6
    lin = merge1(PAIR, [0.8, 0.9], [1, 1], method="linear", iou_threshold=0.5)
    assert lin["count"][0] == 2 and lin["scores64"][0, 1] == D(F(0.8)) * (D(1) - D(0.6))
    assert merge1(PAIR, [0.8, 0.9], [1, 1], method="linear", iou_threshold=0.6)["scores64"][0, 1] == D(F(0.8))        # strict >
    # a decayed score that falls to the threshold or below is never picked
    assert merge1(PAIR, [0.8, 0.9], [1, 1], method="gaussian", score_threshold=0.39)["count"][0] == 1
    assert merge1(PAIR, [0.8, 0.9], [1, 1], method="gaussian", score_threshold=0.38)["count"][0] == 2


def test_ref_labels_separate_unless_class_agnostic():
    for method in ("linear", "gaussian"):
        out = merge1(PAIR, [0.8, 0.9], [0, 1], method=method)
        assert out["count"][0] == 2 and out["scores64"][0].tolist()[:2] == [D(F(0.9)), D(F(0.8))]
        out = merge1(PAIR, [0.8, 0.9], [0, 1], method=method, class_aware=False)
        assert out["count"][0] == 2 and out["scores64"][0, 1] < D(F(0.8)) and out["labels"][0].tolist()[:2] == [1, 0]


def test_ref_a_decay_reorders_the_picks():
    # B overlaps the best box A, C stands alone: hard order is A, B's removal, C; soft order is A, C, then B with what is left of its score
    boxes = [[0, 0, 100, 100], [10, 0, 110, 100], [500, 500, 600, 600]]
    out = merge1(boxes, [0.9, 0.8, 0.7], [0, 0, 0], method="gaussian")
    assert out["source"][0].tolist() == [0, 2, 1, -1, -1] and out["scores"][0, 1] == F(0.7) and out["scores"][0, 2] < F(0.7)
    assert (np.diff(out["scores64"][0, :3]) <= 0).all()
    assert merge1(boxes, [0.9, 0.8, 0.7], [0, 0, 0], method="hard")["source"][0].tolist() == [0, 2, -1, -1, -1]


def test_ref_equal_scores_go_by_position_and_padding_is_zero():
    boxes = [[0, 0, 10, 10], [500, 500, 510, 510], [200, 200, 210, 210], [300, 300, 310, 310]]
    for method in METHODS:
        out = merge1(boxes, [0.5, 0.5, 0.5, 0.01], [0, 0, 0, 0], K_out=6, method=method)
        assert out["source"][0].tolist() == [0, 1, 2, -1, -1, -1] and out["count"][0] == 3
        assert (out["scores"][0, 3:] == 0).all() and (out["labels"][0, 3:] == 0).all() and (out["bboxes"][0, 3:] == 0).all()
        assert merge1(boxes, [0.5, 0.7, 0.5, -0.0], [0, 0, 0, 0], method=method, score_threshold=-1.0)["source"][0].tolist() == [1, 0, 2, 3, -1]
        assert merge1(boxes, [0.5, 0.7, 0.6, 0.4], [0, 0, 0, 0], K_out=2, method=method)["source"][0].tolist() == [1, 2]
        assert merge1(boxes, [0.5, 0.7, 0.6, 0.4], [0, 0, 0, 0], method=method, max_candidates=2)["source"][0].tolist() == [1, 2, -1, -1, -1]


def test_ref_degenerate_boxes_weigh_one():
    boxes = [[0, 0, 0, 0], [0, 0, 0, 0], [5, 5, 5, 50], [np.nan, 0, 0, 0]]
    for method in ("linear", "gaussian"):
        out = merge1(boxes, [0.9, 0.8, 0.7, 0.6], [0, 0, 0, 0], method=method)
        assert out["count"][0] == 4 and out["scores64"][0, :4].tolist() == [D(F(v)) for v in (0.9, 0.8, 0.7, 0.6)]
        assert not np.isnan(out["bboxes"]).any()


# ----------------------------------------------------------------------------- one loop = two steps
def assert_same_picks(one, two, what):
    assert np.array_equal(one["count"], two["count"]), (what, one["count"], two["count"])
    assert np.array_equal(one["source"], two["source"]), (what, np.argwhere(one["source"] != two["source"])[:5].tolist())
    assert np.array_equal(one["labels"], two["labels"]), what
    assert np.array_equal(one["scores64"].view(np.uint64), two["scores64"].view(np.uint64)), what


@pytest.mark.parametrize("class_aware", [True, False])
@pytest.mark.parametrize("method", METHODS)
def test_the_one_loop_rule_is_per_class_soft_nms_then_top_k(method, class_aware):
    """The kernel's form (soft_merge_ref: one loop over all classes, stop at K_out) against the original's (two_step_ref: every class to
    exhaustion, then the K_out best): the same sources, labels and float64 scores.  It holds because scores >= 0 only decay, so a class's
    picks leave in non-increasing order and the global maximum is always some class's next pick."""
    for (N, S, seed) in [(1, 5, 7), (3, 2, 8), (1, 1, 9)]:
        rec, ffv = ref.scale_records(ref.FRAME_SIZES[:N], S)
        boxes, scores, labels = ref.planted_candidates(np.random.default_rng(seed), rec, ffv, 60, n_objects=25)
        for K_out in (20, 100, 400):
            kw = dict(method=method, sigma=0.5, iou_threshold=0.5, score_threshold=0.05, class_aware=class_aware)
            one = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, K_out, **kw)
            two = ref.two_step_ref(boxes, scores, labels, rec, ffv, K_out, **kw)
            assert_same_picks(one, two, (method, class_aware, N, S, K_out))
            m = one["count"]
            for n in range(N):
                assert (np.diff(one["scores64"][n, :m[n]]) <= 0).all()                        # the picks leave in non-increasing order
            assert (m > 0).all()
        # a frame's result depends on its own views only
        if N > 1:
            alone = ref.soft_merge_ref(boxes[ffv[1]:ffv[2]], scores[ffv[1]:ffv[2]], labels[ffv[1]:ffv[2]], rec[ffv[1]:ffv[2]], [0, S], 100, **kw)
            batch = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 100, **kw)
            assert_same_picks(alone, {key: batch[key][1:2] for key in ("count", "source", "labels", "scores64")}, "alone")


def test_the_hard_method_is_the_hard_merge_on_the_restatements():
    for (N, S, seed) in ref.RANDOM_CASES[3:7]:
        boxes, scores, labels, rec, ffv = ref.random_case(N, S, seed)
        for K_out, t, st in ((100, 0.5, 0.05), (17, 0.3, 0.0), (400, 0.7, 0.5)):
            soft = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, K_out, method="hard", iou_threshold=t, score_threshold=st)
            hard = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, K_out, score_threshold=st, match_threshold=t, metric=0)
            for key in ("count", "source", "labels"):
                assert np.array_equal(soft[key], hard[key]), (key, N, S, K_out)
            assert np.array_equal(soft["scores"].view(np.uint32), hard["scores"].view(np.uint32))
            assert np.array_equal(soft["bboxes"].view(np.uint32), hard["bboxes"].view(np.uint32))


# ----------------------------------------------------------------------------- what the gaussian comparisons on the GPU rest on
def test_every_gaussian_case_of_the_gpu_tests_has_its_margin():
    """The device's exp and numpy's differ by a couple of float64 ulp per call, a score sees at most K_out decays: about 300 x 4.4e-16 =
    1.3e-13 of relative difference.  The picks, and the live test against score_threshold, are the same on both sides as long as no
    decision is closer than that: 1e-9 leaves four orders of magnitude.  A case that fails is replaced in soft_nms_ref, not tolerated."""
    worst = np.inf
    for (N, S, seed) in ref.RANDOM_CASES:
        boxes, scores, labels, rec, ffv = ref.random_case(N, S, seed)
        out = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, ref.RANDOM_K_OUT, method="gaussian", **ref.RANDOM_KW)
        assert out["margin"] >= ref.MIN_MARGIN, (N, S, seed, out["margin"])
        assert out["count"].min() >= min(40, ref.RANDOM_K_OUT)                                # the cases are crowded
        worst = min(worst, out["margin"])
    for name, (boxes, scores, labels, rec, ffv, K_out, kw) in ref.edge_cases().items():
        out = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, K_out, method="gaussian", **kw)
        assert out["margin"] >= ref.MIN_MARGIN, (name, out["margin"])
        worst = min(worst, out["margin"])
    boxes, scores, labels, rec, ffv, _, kw = ref.edge_cases()["M=257"]
    for kw2 in ref.DECAY_VARIANTS:
        if kw2["method"] == "gaussian":
            out = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 1000, **dict(kw, **kw2))
            assert out["margin"] >= ref.MIN_MARGIN, (kw2, out["margin"])
            worst = min(worst, out["margin"])
    boxes, scores, labels, rec, ffv = ref.planted_pair()
    out = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 10, method="gaussian", score_threshold=0.05)
    assert out["margin"] >= ref.MIN_MARGIN
    worst = min(worst, out["margin"])
    print(f"smallest gaussian margin over the GPU tests' cases: {worst:.3g}")


def test_the_edge_cases_are_what_they_say():
    cases = ref.edge_cases()
    count = lambda name, **kw: ref.soft_merge_ref(*cases[name][:5], cases[name][5], **dict(cases[name][6], **kw))
    for m in (1, 64, 65, 256, 257):
        assert count(f"M={m}", method="linear")["count"].tolist() == [m]                      # (no pair overlaps by more than 0.5: all are picked)
    out = count("M=2500")
    assert cases["M=2500"][0].shape[:2] == (25, 100) and out["count"].tolist() == [120]
    assert count("K_out=1")["count"].tolist() == [1]
    out = count("distinct classes")
    assert out["count"].tolist() == [300] and np.array_equal(out["scores"][0, :300], np.sort(cases["distinct classes"][1].reshape(-1))[::-1])
    assert count("cap bites")["count"].tolist() == [130] and count("cap bites", max_candidates=4096)["count"].tolist() == [150]
    assert count("0 and 1 candidates")["count"].tolist() == [0, 1] and count("0 and 1 candidates")["source"][1, 0] == 7
    out = count("signed zero and NaN scores")
    zero = out["source"][0][(out["scores"][0] == 0) & (out["source"][0] >= 0)]
    assert len(zero) == 80 and (np.diff(zero) > 0).all() and not np.isnan(out["scores"]).any()
    assert count("signed zero and NaN scores, threshold -0")["scores"][0].min() >= 0
    out = count("NaN and degenerate boxes")
    assert out["count"][0] > 100 and not np.isnan(out["bboxes"]).any() and not np.isnan(out["scores64"]).any()
    boxes, scores, labels, rec, ffv = ref.planted_pair()
    hard = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 10, method="hard", score_threshold=0.05)
    soft = ref.soft_merge_ref(boxes, scores, labels, rec, ffv, 10, method="gaussian", score_threshold=0.05)
    assert hard["count"].tolist() == [1] and soft["count"][0] >= 2 and soft["source"][0, :2].tolist() == [0, 1]
    assert 0.05 < soft["scores"][0, 1] < scores[0, 1]                                         # the second object, decayed by the first
