"""No GPU: the flip-test rule (tests/flip_ref.py) on a hand-written box map, the declarations of cnl_flip_merge_f32 and
cnl_mirror_append_u8, their argument checks, and the refusals of the Python surface."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import flip_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, flip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "centernet-lightning_amd", "configs")
ENTRIES = ("cnl_flip_merge_f32", "cnl_mirror_append_u8")


def test_rule_on_a_hand_written_box_map():
    # [2N = 2, C = 4 (left, top, right, bottom), H = 1, W = 3]: the image's map, then the mirrored image's
    maps = torch.tensor([[[[1.0, 2.0, 3.0]], [[10.0, 20.0, 30.0]], [[100.0, 200.0, 300.0]], [[1000.0, 2000.0, 3000.0]]],
                         [[[5.0, 7.0, 9.0]], [[50.0, 70.0, 90.0]], [[500.0, 700.0, 900.0]], [[5000.0, 7000.0, 9000.0]]]])
    assert tuple(maps.shape) == (2, 4, 1, 3)
    # left at x = mean of the image's left at x and the mirror's RIGHT at W - 1 - x; top and bottom keep their channel
    want_box = torch.tensor([[[[450.5, 351.0, 251.5]], [[50.0, 45.0, 40.0]], [[54.5, 103.5, 152.5]], [[5000.0, 4500.0, 4000.0]]]])
    want_plain = torch.tensor([[[[5.0, 4.5, 4.0]], [[50.0, 45.0, 40.0]], [[500.0, 450.0, 400.0]], [[5000.0, 4500.0, 4000.0]]]])
    assert torch.equal(flip_ref.merge(maps, swap_lr=True), want_box)
    assert torch.equal(flip_ref.merge(maps, swap_lr=False), want_plain)
    got = flip_ref.merge_outputs({"heatmap": maps, "box_2d": maps})
    assert torch.equal(got["heatmap"], want_plain) and torch.equal(got["box_2d"], want_box)
    # the mirror of the merged box map: columns reversed, left and right swapped
    assert torch.equal(flip_ref.mirror_maps({"box_2d": want_box})["box_2d"],
                       torch.tensor([[[[152.5, 103.5, 54.5]], [[40.0, 45.0, 50.0]], [[251.5, 351.0, 450.5]], [[4000.0, 4500.0, 5000.0]]]]))
    u8 = torch.tensor([[[[1, 2], [3, 4], [5, 6]]]], dtype=torch.uint8)                      # [1, 1, 3, 2]
    assert flip_ref.mirror_append(u8).tolist() == [[[[1, 2], [3, 4], [5, 6]]], [[[5, 6], [3, 4], [1, 2]]]]
    assert flip.SWAP_LR == flip_ref.SWAP_LR


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for entry in ENTRIES:
        assert re.search(r"\bint\s+" + entry + r"\s*\(", header), f"{entry} is not declared in include/centernet_gfx950.h"
        assert entry in _lib.EXPORTED_SYMBOLS and hasattr(lib, entry)
    assert "0.5f * ( a[n, c, y, x] + b[n, p(c), y, W - 1 - x] )" in header and "dst[N + n, y, x] = src[n, y, W - 1 - x]" in header
    assert lib.cnl_version() == _lib.ABI_VERSION == 13            # entry points only: no ABI bump,
    assert lib.cnl_sizeof_params(3) == 0                          # and the descriptor is not a registered params struct
    assert ctypes.sizeof(_lib.FlipMap) == 128
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert cl.flip_merge is flip.flip_merge and cl.mirror_append_uint8 is flip.mirror_append_uint8
    assert "flip_merge" in cl.__all__ and "mirror_append_uint8" in cl.__all__
    for name in ("forward", "get_encoded_outputs", "forward_uint8", "detect_frames", "detect_tiled"):
        assert inspect.signature(getattr(cl.CenterNet, name)).parameters["flip_test"].default is False, name


def fake_map(C=4, swap_lr=0, a=0x10000, b=0x20000, dst=0x30000):
    """A descriptor with fake pointers (never dereferenced: every call made with it fails validation or is a no-op)."""
    m = _lib.FlipMap()
    m.a, m.b, m.dst, m.C, m.swap_lr = a, b, dst, C, swap_lr
    m.a_sc = m.b_sc = m.d_sc = 1
    return m


def test_entry_points_validate_arguments_without_a_device():
    lib = _lib.load()
    E = _lib.CNL_E_BAD_ARG
    for C in (0, 5, -1):
        assert lib.cnl_mirror_append_u8(0x10000, 0x20000, 1, 2, 2, C, None) == E and f"C = {C}" in _lib.last_error()
    assert lib.cnl_mirror_append_u8(0x10000, 0x20000, -1, 2, 2, 3, None) == E and "negative" in _lib.last_error()
    assert lib.cnl_mirror_append_u8(None, 0x20000, 1, 2, 2, 3, None) == E and "null pointer" in _lib.last_error()
    assert lib.cnl_mirror_append_u8(0x10000, 0x20000, 32768, 32768, 1, 1, None) == E and "2^31" in _lib.last_error()
    for shape in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):               # no pixels: a no-op whose pointers are not looked at
        assert lib.cnl_mirror_append_u8(None, None, *shape, 3, None) == 0

    def merge(maps, n=None, N=1, H=2, W=2):
        table = (_lib.FlipMap * max(len(maps), 1))(*maps)
        return lib.cnl_flip_merge_f32(table, len(maps) if n is None else n, N, H, W, None)

    assert merge([fake_map(C=0)]) == E and "C = 0" in _lib.last_error()
    assert merge([fake_map(), fake_map(C=-3)]) == E and "map 1" in _lib.last_error()
    assert merge([fake_map(C=5, swap_lr=1)]) == E and "swap_lr" in _lib.last_error()
    assert merge([fake_map()], n=4) == E and "n_maps" in _lib.last_error()
    assert merge([fake_map()], n=-1) == E and "n_maps" in _lib.last_error()
    assert merge([fake_map()], N=-1) == E and "negative" in _lib.last_error()
    assert lib.cnl_flip_merge_f32(None, 1, 1, 2, 2, None) == E and "null pointer" in _lib.last_error()
    for name in ("a", "b", "dst"):
        assert merge([fake_map(**{name: None})]) == E and "null pointer" in _lib.last_error(), name
        assert merge([fake_map(**{name: 0x10002})]) == E and "aligned" in _lib.last_error(), name
    assert merge([fake_map(C=80)], N=64, H=1024, W=1024) == E and "2^31" in _lib.last_error()
    assert lib.cnl_flip_merge_f32(None, 0, 1, 2, 2, None) == 0     # no maps, no pixels: no-ops
    for shape in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):
        assert merge([fake_map(a=None, b=None, dst=None)], N=shape[0], H=shape[1], W=shape[2]) == 0


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        flip.mirror_append_uint8(torch.zeros((2, 4, 4, 3), dtype=torch.uint8))
    maps = {"heatmap": torch.zeros((2, 3, 4, 4)), "box_2d": torch.zeros((2, 4, 4, 4))}
    with pytest.raises(RuntimeError, match="HIP devices only"):
        flip.flip_merge(maps, 1)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        flip.flip_merge(cl.DetectionOutput(**maps), 1)
    model = cl.build_centernet(os.path.join(CONFIGS, "resnet34_simple.yaml"))
    with pytest.raises(RuntimeError):
        model.forward(torch.zeros((1, 3, 64, 64)), flip_test=True)
    with pytest.raises(RuntimeError):
        model(torch.zeros((1, 3, 64, 64)), flip_test=True)
    with pytest.raises(RuntimeError):
        model.get_encoded_outputs(torch.zeros((1, 3, 64, 64)), flip_test=True)
    with pytest.raises(RuntimeError):
        model.forward_uint8(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), flip_test=True)


def test_flip_merge_refuses_what_is_not_a_doubled_batch():
    with pytest.raises(ValueError, match="6 outputs"):            # an odd batch cannot be the images and their mirrors
        flip.flip_merge({"heatmap": torch.zeros((5, 3, 4, 4)), "box_2d": torch.zeros((5, 4, 4, 4))}, 3)
    with pytest.raises(ValueError, match="2 outputs"):
        flip.flip_merge({"heatmap": torch.zeros((3, 3, 4, 4))}, 1)
    with pytest.raises(ValueError):
        flip.flip_merge({"heatmap": torch.zeros((2, 3, 4, 4)), "box_2d": torch.zeros((4, 4, 4, 4))}, 1)
    with pytest.raises(ValueError, match="map size"):
        flip.flip_merge({"heatmap": torch.zeros((2, 3, 4, 4)), "box_2d": torch.zeros((2, 4, 4, 8))}, 1)
    with pytest.raises(ValueError, match="4 channels"):
        flip.flip_merge({"box_2d": torch.zeros((2, 5, 4, 4))}, 1)
    with pytest.raises(ValueError):
        flip.flip_merge({"heatmap": torch.zeros((2, 3, 4, 4), dtype=torch.float64)}, 1)
    with pytest.raises(ValueError):
        flip.flip_merge({"heatmap": torch.zeros((2, 3, 4, 4))}, -1)
    with pytest.raises(TypeError):
        flip.flip_merge([torch.zeros((2, 3, 4, 4))], 1)
    with pytest.raises(ValueError):
        flip.mirror_append_uint8(torch.zeros((2, 4, 4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError):
        flip.mirror_append_uint8(torch.zeros((2, 4, 4, 3)))
