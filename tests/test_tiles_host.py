"""No GPU: the tile grid rule, the merge's C-ABI declarations and argument checks, the Python surface's refusals, and the numpy
restatement of the merge rule (tests/tiled_ref.py) on hand-made cases."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import letterbox_ref
import tiled_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnl_merge_tiles_workspace_bytes", "cnl_merge_tiles_f32")
F = np.float32


# ----------------------------------------------------------------------------- geometry
def test_worked_example_1080p():
    grid = cl.tile_grid(1080, 1920, 512, 512, 0.2)
    assert round(512 * 0.2) == 102
    assert [x0 for (y0, x0, _, _) in grid if y0 == 0] == [0, 410, 820, 1230, 1408]
    assert sorted({y0 for (y0, _, _, _) in grid}) == [0, 410, 568]
    assert grid == [(y0, x0, 512, 512) for y0 in (0, 410, 568) for x0 in (0, 410, 820, 1230, 1408)]       # row-major
    assert len(grid) == 15 and grid == tiled_ref.tile_grid_ref(1080, 1920, 512, 512, 0.2)
    assert cl.tile_grid(1080, 1920) == grid                                                               # the defaults
    rec, ffv, views = tiled_ref.view_records([(1080, 1920)], 512, 512, 0.2, True, letterbox_ref.geometry)
    assert ffv == [0, 16] and views[-1] == (0, 0, 0, 1080, 1920)                                          # 15 tiles + the full view
    assert rec[-1][:6] == (1920, 1080, 0, 0, 0, 112) and rec[-1][6] == F(512) / F(1920) and rec[-1][7] == F(288) / F(1080)


SWEEP = sorted(set(list(range(1, 40)) + [255, 256, 257, 300, 409, 410, 411, 511, 512, 513, 607, 608, 609, 614, 615, 720, 922, 923, 1000, 1023,
                                         1024, 1025, 1080, 1087, 1088, 1089, 1280, 1919, 1920, 2047, 2048, 2160, 2199, 2200]))


@pytest.mark.parametrize("overlap", [0, 0.2, 0.5])
@pytest.mark.parametrize("tile_h,tile_w", [(256, 256), (512, 512), (608, 1088)])
def test_grid_properties(tile_h, tile_w, overlap):
    assert SWEEP[0] == 1 and SWEEP[-1] == 2200
    for size in SWEEP:
        for along_x in (True, False):
            tile = tile_w if along_x else tile_h
            grid = cl.tile_grid(7, size, tile_h, tile_w, overlap) if along_x else cl.tile_grid(size, 7, tile_h, tile_w, overlap)
            spans = [(x0, tw) if along_x else (y0, th) for (y0, x0, th, tw) in grid]
            ov = round(tile * overlap)
            step = tile - ov
            n = 1 if size <= tile else math.ceil((size - tile) / step) + 1
            assert len(spans) == n, (size, tile, overlap)
            covered = np.zeros(size, dtype=bool)
            for (a, length) in spans:
                assert 0 <= a and a + length <= size and 1 <= length <= tile             # inside the frame
                assert length == (tile if size > tile else size)
                covered[a:a + length] = True
            assert covered.all(), (size, tile, overlap)                                   # the union covers every pixel
            for (a, la), (b, lb) in zip(spans, spans[1:]):
                assert b > a and a + la - b >= ov, (size, tile, overlap, spans)          # consecutive tiles overlap by at least ov
    for h, w in [(1080, 1920), (2160, 3840), (300, 400), (513, 1000), (1, 1)]:
        grid = cl.tile_grid(h, w, tile_h, tile_w, overlap)
        assert grid == tiled_ref.tile_grid_ref(h, w, tile_h, tile_w, overlap)
        assert grid == sorted(grid)                                                       # row-major: y0 first, then x0
        seen = np.zeros((h, w), dtype=bool)
        for (y0, x0, th, tw) in grid:
            seen[y0:y0 + th, x0:x0 + tw] = True
        assert seen.all()


@pytest.mark.parametrize("args", [(0, 5, 512, 512, 0.2), (5, 0, 512, 512, 0.2), (-3, 5, 512, 512, 0.2), (5, 5, 0, 512, 0.2), (5, 5, 512, 500, 0.2),
                                  (5, 5, 100, 512, 0.2), (5, 5, -32, 32, 0.2), (5.0, 5, 512, 512, 0.2), (5, 5, 512.0, 512, 0.2),
                                  (True, 5, 512, 512, 0.2), (5, 5, 512, True, 0.2), (5, 5, 512, 512, 0.51), (5, 5, 512, 512, -0.1),
                                  (5, 5, 512, 512, "0.2"), (5, 5, 512, 512, None), (5, 5, 512, 512, True), (5, 5, 512, 512, float("nan"))])
def test_grid_rejects_bad_arguments(args):
    with pytest.raises(ValueError):
        cl.tile_grid(*args)


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in include/centernet_gfx950.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # entry points only: no ABI bump, no new params struct
    assert lib.cnl_sizeof_params(3) == 0
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
        assert set(ENTRY_POINTS) <= defined


def test_merge_validates_arguments_without_a_device():
    lib = _lib.load()
    E = _lib.CNL_E_BAD_ARG
    fake = 0x10000          # never dereferenced: every call below fails validation first

    def call(boxes=fake, scores=fake, labels=fake, views=fake, ffv=fake, N=1, V=16, k=100, K_out=300, cap=4096, st=0.1, mt=0.5, metric=0, ca=1,
             ob=fake, os_=fake, ol=fake, osrc=fake, oc=fake, ws=fake, ws_bytes=1 << 40):
        return lib.cnl_merge_tiles_f32(boxes, scores, labels, views, ffv, N, V, k, K_out, cap, st, mt, metric, ca, ob, os_, ol, osrc, oc, ws, ws_bytes, None)

    assert call(boxes=None, scores=None, labels=None, views=None, ffv=None, ob=None, os_=None, ol=None, osrc=None, oc=None, ws=None) == E
    assert "null" in _lib.last_error()
    for name in ("boxes", "scores", "labels", "views", "ffv", "ob", "os_", "ol", "osrc", "oc"):
        assert call(**{name: None}) == E, name
    assert call(N=-1) == E and "N = -1" in _lib.last_error()
    assert call(V=-1) == E and call(k=0) == E and call(K_out=0) == E
    assert call(cap=0) == E and call(cap=16385) == E and "max_candidates" in _lib.last_error()
    assert call(metric=2) == E and "metric" in _lib.last_error()
    assert call(st=float("nan")) == E and call(mt=float("nan")) == E
    assert call(boxes=fake + 4) == E and "aligned" in _lib.last_error()
    assert call(ws=None) == _lib.CNL_E_WORKSPACE and call(ws_bytes=16) == _lib.CNL_E_WORKSPACE
    assert call(N=0, boxes=None, scores=None, labels=None, views=None, ffv=None, ob=None, os_=None, ol=None, osrc=None, oc=None, ws=None, ws_bytes=0) == 0
    # the workspace grows with the candidates, not with N x max_candidates^2
    small, big = lib.cnl_merge_tiles_workspace_bytes(1, 16, 100, 4096), lib.cnl_merge_tiles_workspace_bytes(32, 512, 100, 4096)
    assert 0 < small < big <= 64 << 20
    assert lib.cnl_merge_tiles_workspace_bytes(1, 16, 100, 0) == 0 and lib.cnl_merge_tiles_workspace_bytes(-1, 16, 100, 4096) == 0


def test_python_surface_rejects_cpu_and_malformed_input():
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    for name in ("tile_uint8", "merge_tiles", "detect_tiled"):
        assert callable(getattr(model, name))
    for name in ("tile_grid", "tile_uint8", "merge_tiles", "TileGeometry"):
        assert hasattr(cl, name) and name in cl.__all__
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        cl.tile_uint8([frame], 32, 32)                                  # CPU frames: no fallback
    with pytest.raises(RuntimeError):
        model.detect_tiled(frame[None])
    with pytest.raises(RuntimeError):
        cl.merge_tiles(torch.zeros((1, 4, 4)), torch.zeros((1, 4)), torch.zeros((1, 4), dtype=torch.int64), None)
    with pytest.raises(ValueError):
        cl.tile_uint8([], 32, 32)
    with pytest.raises(ValueError):
        cl.tile_uint8(frame, 32, 32)                                    # a tensor must be 4-D
    with pytest.raises(ValueError):
        model.detect_tiled([frame], batch=0)


def _malformed_detections():
    """(what is wrong, bboxes, scores, labels): one argument of a well-formed CPU triple replaced per row; the last row is the triple itself."""
    good = (torch.zeros((2, 4, 4)), torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int64))

    def swap(i, value):
        return tuple(value if j == i else t for j, t in enumerate(good))
    return [("numpy array instead of tensor", *swap(0, np.zeros((2, 4, 4), dtype=F))),
            ("None", *swap(1, None)),
            ("float64 boxes", *swap(0, good[0].double())),
            ("fp16 scores", *swap(1, good[1].half())),
            ("int32 labels", *swap(2, good[2].int())),
            ("rank-2 boxes", *swap(0, torch.zeros((2, 4)))),
            ("last dimension of 5", *swap(0, torch.zeros((2, 4, 5)))),
            ("scores of another shape", *swap(1, torch.zeros((2, 3)))),
            ("labels of another shape", *swap(2, torch.zeros((4, 2), dtype=torch.int64))),
            ("a well-formed CPU triple", *good)]


def test_merges_keep_their_exception_types_for_malformed_detections():
    """merge_tiles looks at where the tensors live first, so without a device every row is a RuntimeError; merge_soft looks at what they
    are first (ValueError) and only then at where they live, so only the well-formed CPU triple gets that far."""
    _lib.load()
    model = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_simple.yaml"))
    for what, bboxes, scores, labels in _malformed_detections():
        soft_raises = RuntimeError if what == "a well-formed CPU triple" else ValueError
        for merge, raises in ((cl.merge_tiles, RuntimeError), (model.merge_tiles, RuntimeError), (cl.merge_soft, soft_raises),
                              (model.merge_soft, soft_raises)):
            with pytest.raises((RuntimeError, ValueError)) as caught:
                merge(bboxes, scores, labels, None)
            assert type(caught.value) is raises, f"{merge.__qualname__} on {what}: {caught.value!r}"


# ----------------------------------------------------------------------------- the restated rule on hand-made cases
TILE = (1000, 1000, 0, 0, 0, 0, F(1), F(1))          # one view that is the frame: boxes map to themselves


def merge1(boxes, scores, labels, K_out=5, records=None, ffv=None, **kw):
    boxes = np.asarray(boxes, dtype=F)
    V = 1 if boxes.ndim == 2 else boxes.shape[0]
    boxes, scores, labels = boxes.reshape(V, -1, 4), np.asarray(scores, dtype=F).reshape(V, -1), np.asarray(labels).reshape(V, -1)
    return tiled_ref.merge_ref(boxes, scores, labels, records or [TILE] * V, ffv or [0, V], K_out, **kw)


def test_ref_same_label_iou_06_leaves_one():
    # [0,100] x [0,100] and [25,125] x [0,100]: inter 7500, union 12500 -> IoU 0.6
    boxes, labels = [[0, 0, 100, 100], [25, 0, 125, 100]], [1, 1]
    out = merge1(boxes, [0.8, 0.9], labels)
    assert out["count"][0] == 1 and out["source"][0].tolist() == [1, -1, -1, -1, -1] and out["scores"][0, 0] == F(0.9)
    assert merge1(boxes, [0.8, 0.9], labels, match_threshold=0.6)["count"][0] == 2          # strict >: IoU 0.6 does not exceed 0.6
    assert merge1(boxes, [0.8, 0.9], labels, match_threshold=0.59)["count"][0] == 1


def test_ref_labels_separate_unless_class_agnostic():
    boxes = [[0, 0, 100, 100], [25, 0, 125, 100]]
    assert merge1(boxes, [0.8, 0.9], [0, 1])["count"][0] == 2
    out = merge1(boxes, [0.8, 0.9], [0, 1], class_aware=False)
    assert out["count"][0] == 1 and out["labels"][0, 0] == 1


def test_ref_cut_box_needs_ios():
    # a box cut by a tile edge, [0,30] x [0,100], inside the whole box [0,100] x [0,100]: IoU 0.3, IoS 1.0
    boxes = [[0, 0, 100, 100], [0, 0, 30, 100]]
    assert merge1(boxes, [0.9, 0.8], [0, 0], metric=0)["count"][0] == 2
    out = merge1(boxes, [0.9, 0.8], [0, 0], metric=1)
    assert out["count"][0] == 1 and out["source"][0, 0] == 0


def test_ref_equal_scores_go_by_candidate_number():
    boxes = [[0, 0, 10, 10], [500, 500, 510, 510], [0, 0, 10, 10], [200, 200, 210, 210]]
    out = merge1(boxes, [0.5, 0.5, 0.5, 0.5], [0, 0, 0, 0])
    assert out["source"][0].tolist() == [0, 1, 3, -1, -1] and out["count"][0] == 3            # candidate 2 duplicates candidate 0
    out = merge1(boxes, [0.5, 0.7, 0.5, -0.0], [0, 0, 0, 0], score_threshold=-1.0)
    assert out["source"][0].tolist() == [1, 0, 3, -1, -1]


def test_ref_cap_and_padding():
    boxes = [[100 * i, 0, 100 * i + 50, 50] for i in range(6)]
    scores = [0.9, 0.2, 0.8, 0.05, 0.7, 0.6]
    out = merge1(boxes, scores, [0] * 6, K_out=8)
    assert out["count"][0] == 5 and out["source"][0].tolist() == [0, 2, 4, 5, 1, -1, -1, -1]  # 0.05 fails the threshold
    assert (out["scores"][0, 5:] == 0).all() and (out["labels"][0, 5:] == 0).all() and (out["bboxes"][0, 5:] == 0).all()
    out = merge1(boxes, scores, [0] * 6, K_out=8, max_candidates=3)
    assert out["count"][0] == 3 and out["source"][0].tolist() == [0, 2, 4, -1, -1, -1, -1, -1]
    out = merge1(boxes, scores, [0] * 6, K_out=2)
    assert out["count"][0] == 2 and out["source"][0].tolist() == [0, 2]
    out = merge1(boxes, scores, [0] * 6, score_threshold=0.95)
    assert out["count"][0] == 0 and (out["source"][0] == -1).all()


def test_ref_maps_views_into_the_frame_and_numbers_candidates_per_frame():
    # frame 0: 1080 x 1920, a tile at (410, 1408) and the full view; frame 1: one tile.  The same object seen in both views of frame 0.
    rec, ffv, _ = tiled_ref.view_records([(1080, 1920)], 512, 512, 0.2, True, letterbox_ref.geometry)
    tile, full = rec[9], rec[15]
    assert tile[:4] == (1920, 1080, 1408, 410)
    in_tile = np.array([[10, 20, 110, 220]], dtype=F)
    in_frame = tiled_ref.map_boxes_ref(in_tile, tile)
    assert in_frame.tolist() == [[1418, 430, 1518, 630]]
    sx, sy = full[6], full[7]
    in_full = np.array([[F(1418) * sx, F(430) * sy + F(112), F(1518) * sx, F(630) * sy + F(112)]], dtype=F)
    back = tiled_ref.map_boxes_ref(in_full, full)
    assert np.abs(back - in_frame).max() < 1e-3
    assert tiled_ref.map_boxes_ref(np.array([[-2000, -5, 600, 600]], dtype=F), rec[14]).tolist() == [[0, 563, 1920, 1080]]      # clamped to the FRAME
    out = tiled_ref.merge_ref(np.stack([in_tile, in_full, in_tile]), np.array([[0.5], [0.6], [0.4]], dtype=F), np.zeros((3, 1), np.int64),
                              [tile, full, TILE], [0, 2, 3], 4)
    assert out["count"].tolist() == [1, 1] and out["source"][:, 0].tolist() == [1, 0]       # frame 1's candidate is its own number 0
