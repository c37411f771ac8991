"""GPU: the detection side of the C ABI under guards — strided views, guarded outputs, exactly sized workspaces.

The value tests of these entries (test_gpu_decode.py, test_gpu_tracker.py, test_gpu_track_streams.py, test_gpu_tiles.py, test_gpu_coco_eval.py,
test_gpu_letterbox.py) hand the kernels packed, exactly sized, allocation-aligned torch tensors and read back the elements they expect.  Here every
launch goes through the C ABI itself with

    inputs    logical views of wider storage (tests/strided_io.py: StridedView) surrounded by +inf / NaN, so that a read outside the view changes a result;
    outputs   separate GuardedBytes buffers at exactly the alignment include/centernet_gfx950.h states for them, sentinel before, after and between;
    workspace exactly as many bytes as the *_bytes query promises, at exactly its stated alignment;

and afterwards (a) the result equals the oracle the entry's own tests use, bit for bit, (b) nothing outside the declared output bytes changed, (c) every
input allocation is bit for bit what it was, (d) where a packed control exists, the strided result equals it bit for bit.  No tolerance is introduced.
The last test asserts that the decode's (stage-1 kernel, vector width, top-k key storage) forms that ran UNDER A NON-PACKED LAYOUT contain a written-down
list (cnl_decode_forms, the launcher's own decision)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import decode_ref
import letterbox_ref
import lsap_ref
import tiled_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, _track_host
from strided_io import GuardedBytes, StridedView, record_mask

pytestmark = pytest.mark.gpu

S1_NAMES = {1: "cminor", 2: "c8", 3: "planes", 4: "generic"}
TK_NAMES = {0: "regs16", 1: "lds32", 2: "regs48", 3: "lds16", 4: "memory"}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(g, mask=None):
    ok, msg = g.verdict(mask)
    assert ok, msg


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ====================================================================================================================== decode
# (id, N, C, H, W, k, nms, E, heat layout, box layout, reid layout, kind, emb alignment)
# The embeddings' 16-byte path (e_vec4 in topk_kernel) needs reid_sc == 1, E % 4 == 0, the other reid strides % 4 == 0, reid 16-byte aligned and emb 16-byte
# aligned.  Five cases fail exactly ONE of these each, everything else allowing the path (so that dropping a clause from the kernel gathers wrong elements
# or runs a misaligned 16-byte access under guards, not the scalar loop): cm2_by_base8 (channel stride 2), cm1_of_c8_by_base4 (E = 6), cm1_by_odd_ld (pixel
# stride 14), cm1_by_base4 (base at 4 bytes) — each with emb at 16 — and topk_regs48 (emb at exactly 4); c8_strip4_wide passes every clause.  The test
# works the failing clauses out of each launch's own pointers, and the module's last test requires all six sets.
# kind: "ring" scores in [0, 0.5) with the border ring of every class raised by 0.5, so that the reference's winners sit on all four edges and any
# read of the +inf / NaN outside the view would beat or kill them; "signed" (one class, k == H * W) mostly negative scores, ring raised by 0.3: the negative peaks
# on the border exist only because the pool pads with -inf (kat_signed's point), and with k == H * W every one of them is in the output.
DECODE_CASES = [
    # stage 1, C % 8 == 0: both strip heights (16 rows from 256 workgroups on: 8 images x 2 tiles of 64 pixels x 16 strips)
    ("c8_strip4_wide", 2, 8, 24, 20, 50, 3, 8, "nhwc_wide", "nchw_window", "nhwc_wide", "ring", 16),
    ("c8_strip16_wide", 8, 8, 241, 70, 100, 3, 0, "nhwc_wide", "nhwc", None, "ring", 4),
    ("c8_every_other_image", 2, 16, 17, 33, 37, 5, 0, "batch_every_other", "nhwc_ld3", None, "ring", 4),
    ("c8_every_other_pixel", 2, 8, 12, 16, 192, 7, 0, "every_other_pixel_nhwc", "every_other_pixel_nchw", None, "ring", 4),
    ("c8_batch_slice_nopool", 3, 24, 9, 13, 117, 1, 0, "batch_slice", "batch_slice_nchw", None, "ring", 4),
    # channel-minor: the width C allows (12 -> 4, 6 -> 2, 5 -> 1) ...
    ("cm4_by_C", 2, 12, 19, 23, 33, 1, 3, "nhwc_wide", "nchw", "nhwc", "ring", 4),
    ("cm2_by_C", 2, 6, 11, 27, 29, 7, 0, "nhwc_wide", "nhwc_wide", None, "ring", 4),
    ("cm1_by_C", 2, 5, 13, 9, 21, 3, 0, "batch_slice", "nchw_window_odd", None, "ring", 4),
    # ... and the width the strides / the base pointer leave of a C that allows 4
    ("cm2_by_base8", 2, 12, 10, 21, 40, 3, 8, "nhwc_off2", "nhwc", "every_other_channel", "ring", 16),
    ("cm1_by_base4", 2, 12, 10, 21, 40, 5, 8, "nhwc_off1", "nhwc", "nhwc+1+4", "ring", 16),
    ("cm1_by_odd_ld", 1, 12, 9, 14, 126, 3, 8, "nhwc_ld3", "nchw", "nhwc+4+6", "ring", 16),
    ("cm1_of_c8_by_base4", 2, 8, 16, 9, 25, 3, 6, "nhwc_off1", "nhwc_wide", "nhwc+0+2", "ring", 16),
    ("cm1_signed_kfull", 2, 1, 7, 9, 63, 3, 0, "nhwc_wide", "nhwc", None, "signed", 4),
    # class planes on a window of a wider buffer, every pool
    ("planes_window_C7", 2, 7, 9, 60, 50, 3, 3, "nchw_window", "nhwc", "nhwc", "ring", 4),
    ("planes_window_C16_5x5", 1, 16, 33, 68, 77, 5, 0, "nchw_window", "nchw_window", None, "ring", 4),
    ("planes_window_C80_7x7", 1, 80, 8, 64, 30, 7, 0, "nchw_window", "nchw", None, "ring", 4),
    ("planes_window_nopool", 2, 4, 16, 132, 64, 1, 0, "nchw_window", "nchw", None, "ring", 4),
    ("planes_batch_slice_kfull", 2, 8, 7, 8, 56, 3, 0, "batch_slice_nchw", "batch_slice", None, "ring", 4),
    # generic: what is left of the class planes on an odd pitch, doubled pixel strides
    ("generic_odd_pitch", 2, 7, 9, 60, 50, 3, 8, "nchw_window_odd", "nhwc", "nchw_window_odd", "ring", 4),
    ("generic_every_other_pixel", 2, 4, 12, 16, 61, 5, 0, "every_other_pixel_nchw", "every_other_pixel_nhwc", None, "ring", 4),
    ("generic_odd_pitch_signed_kfull", 2, 1, 9, 11, 99, 3, 0, "nchw_window_odd", "nchw", None, "signed", 4),
    # the top-k's key storage above 16384 pixels: LDS, 48 registers, 16-bit LDS, memory
    ("topk_lds32", 2, 2, 150, 150, 300, 3, 0, "nhwc_wide", "nhwc", None, "ring", 4),
    ("topk_regs48", 1, 4, 152, 272, 1000, 3, 64, "nchw_window", "nhwc", "nhwc_wide", "ring", 4),
    ("topk_lds16", 2, 2, 199, 201, 511, 3, 0, "nhwc_ld3", "nchw", None, "ring", 4),
    ("topk_memory", 2, 2, 224, 224, 120, 3, 0, "every_other_pixel_nhwc", "nhwc", None, "ring", 4),
]
_DECODE_IDS = [c[0] for c in DECODE_CASES]


def _decode_data(case):
    """(heat, box, reid or None) as CPU tensors, seeded by the case."""
    name, N, C, H, W, k, nms, E, hl, bl, rl, kind, _ = case
    g = torch.Generator().manual_seed(N * 7 + C * 1000 + H * 31 + W + k + nms)
    heat = torch.rand(N, C, H, W, generator=g) * 0.5
    ring = torch.zeros(H, W)
    ring[0, :] = ring[-1, :] = 1
    ring[:, 0] = ring[:, -1] = 1
    if kind == "signed":
        heat = heat * 2 - 0.8 + 0.3 * ring                # interior in [-0.8, 0.2), border in [-0.5, 0.5)
    else:
        heat = heat + 0.5 * ring
    box = torch.rand(N, 4, H, W, generator=g) * 7 - 0.5   # a few negative offsets: the clamp
    reid = torch.randn(N, E, H, W, generator=g) if E else None
    return heat, box, reid


_REF = {}


def _decode_ref(case):
    """The oracle's output of a case, computed once; asserts the condition that makes an outside read visible."""
    name, N, C, H, W, k, nms, E = case[:8]
    if name not in _REF:
        heat, box, reid = _decode_data(case)
        ref = decode_ref.decode_detections(heat.numpy(), box.numpy(), k, nms, reid=reid.numpy() if E else None)
        idx = ref["indices"]
        y, x = idx // W, idx % W
        for n in range(N):
            assert (y[n] == 0).any() and (y[n] == H - 1).any() and (x[n] == 0).any() and (x[n] == W - 1).any(), \
                f"{name}: the reference's winners of image {n} do not touch all four edges — the case would not see an outside read"
        if case[11] == "signed":
            border = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
            assert (ref["scores"][border] < 0).any(), f"{name}: no negative peak on the border — the -inf padding is not exercised"
        _REF[name] = ref
    return _REF[name]


def _decode_params(case, heat, box, reid, outs, ws, ws_bytes):
    name, N, C, H, W, k, nms, E = case[:8]
    p = _lib.DecodeParams()
    p.heat = heat.ptr
    p.heat_sn, p.heat_sc, p.heat_sh, p.heat_sw = heat.strides
    p.box = box.ptr
    p.box_sn, p.box_sc, p.box_sh, p.box_sw = box.strides
    if E:
        p.reid = reid.ptr
        p.reid_sn, p.reid_sc, p.reid_sh, p.reid_sw = reid.strides
        p.emb = outs["embeddings"].ptr
    p.N, p.C, p.H, p.W, p.E = N, C, H, W, E
    p.k, p.nms_kernel = k, nms
    p.normalize_boxes, p.box_log, p.box_multiplier, p.stride = 0, 0, 1.0, 4.0
    p.scores, p.indices, p.labels, p.boxes = outs["scores"].ptr, outs["indices"].ptr, outs["labels"].ptr, outs["boxes"].ptr
    p.workspace, p.workspace_bytes = ws.ptr, ws_bytes
    return p


_OUT_SPEC = {"scores": (4, 4, torch.float32), "indices": (8, 8, torch.int64), "labels": (8, 8, torch.int64), "boxes": (16, 4, torch.float32)}


def _decode_outputs(case, device, sentinel=0xA5):
    """Separate guarded outputs at the header's alignment (their element's; emb at case[12]) and a workspace of exactly the promised size at exactly 16."""
    name, N, C, H, W, k, nms, E = case[:8]
    outs = {key: GuardedBytes(N * k * per, align=al, device=device, sentinel=sentinel, name=f"{name}.{key}") for key, (per, al, _) in _OUT_SPEC.items()}
    if E:
        outs["embeddings"] = GuardedBytes(N * k * E * 4, align=case[12], device=device, sentinel=sentinel, name=f"{name}.emb")
    ws_bytes = int(_lib.load().cnl_decode_workspace_bytes(N, H, W))
    ws = GuardedBytes(ws_bytes, align=16, device=device, sentinel=sentinel, name=f"{name}.workspace")
    return outs, ws, ws_bytes


def _decode_forms(p):
    s1, vec, strip, tk = (ctypes.c_int32(-1) for _ in range(4))
    rc = _lib.load().cnl_decode_forms(ctypes.byref(p), ctypes.byref(s1), ctypes.byref(vec), ctypes.byref(strip), ctypes.byref(tk))
    assert rc == 0, _lib.last_error()
    return s1.value, vec.value, strip.value, tk.value


def _vec_cause(case, form):
    """Why the channel-minor kernel runs at its width: "C" when C alone allows no more, else "layout" (a stride or the base pointer took it away)."""
    C = case[2]
    by_c = 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)
    return "C" if form[1] == by_c else "layout"


def _decode_results(case, outs):
    name, N, C, H, W, k, nms, E = case[:8]
    o = {key: outs[key].result(dt, (N, k, 4) if key == "boxes" else (N, k)).numpy() for key, (_, _, dt) in _OUT_SPEC.items()}
    if E:
        o["embeddings"] = outs["embeddings"].result(torch.float32, (N, k, E)).numpy()
    return o


def _run_decode(case, layouts, poison, device="cuda", sentinel=0xA5):
    """One guarded launch -> (outputs as numpy, forms).  Checks (b) and (c)."""
    hl, bl, rl = layouts
    E = case[7]
    heat_t, box_t, reid_t = _decode_data(case)
    heat = StridedView(heat_t, hl, poison, device, "heat")
    box = StridedView(box_t, bl, "nan", device, "box")
    reid = StridedView(reid_t, rl, "nan", device, "reid") if E else None
    outs, ws, ws_bytes = _decode_outputs(case, device, sentinel)
    p = _decode_params(case, heat, box, reid, outs, ws, ws_bytes)
    forms = _decode_forms(p)
    rc = _lib.load().cnl_decode_f32(ctypes.byref(p), _stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for g in list(outs.values()) + [ws]:
        _ok(g)
    assert heat.unchanged() and box.unchanged() and (reid is None or reid.unchanged()), "an input allocation was written"
    return _decode_results(case, outs), forms + (_evec4_failures(reid, outs["embeddings"].ptr, E) if E else None,)


def _evec4_failures(reid, emb_ptr, E):
    """The clauses of topk_kernel's e_vec4 that a launch fails, in the kernel's order."""
    sn, sc, sh, sw = reid.strides
    checks = (("channel stride", sc == 1), ("E % 4", E % 4 == 0), ("strides % 4", (sn | sh | sw) % 4 == 0), ("reid base", reid.ptr % 16 == 0), ("emb base", emb_ptr % 16 == 0))
    return tuple(name for name, ok in checks if not ok)


def _same(o, ref, keys=None):
    for key in keys or ref:
        assert np.array_equal(_bits(o[key]), _bits(ref[key])), key


# Module state filled by the parametrised test below and read by the module's LAST test, as in test_gpu_strided_io.py: the coverage test means something only
# when the whole module runs in one process in file order (the way the suite runs it).
DECODE_REACHED = set()          # (stage-1 name, vec, cause, strip, top-k name, heat layout) of the launches that passed under a non-packed heat layout
EVEC4_REACHED = set()           # the sets of e_vec4 clauses that the launches with embeddings failed
_CONTROL = {}                   # case name -> the packed control's outputs (computed once, under whichever poison runs first: a packed view has no outside)


@pytest.mark.parametrize("poison", ["inf", "nan"])
@pytest.mark.parametrize("case", DECODE_CASES, ids=_DECODE_IDS)
def test_decode_of_strided_views_into_guarded_outputs(case, poison):
    name = case[0]
    ref = _decode_ref(case)
    o, form = _run_decode(case, case[8:11], poison)
    _same(o, ref)                                                      # (a)
    if name not in _CONTROL:                                           # (d): the packed control, once per case, under the other sentinel byte
        packed = ("nhwc" if case[8].startswith(("nhwc", "batch", "every")) and not case[8].endswith("nchw") else "nchw",) * 3
        _CONTROL[name], _ = _run_decode(case, packed, poison, sentinel=0x3C)
    _same(o, _CONTROL[name])
    assert not StridedView(torch.zeros(1, 1, 1, 1), case[8]).packed
    if case[7]:
        EVEC4_REACHED.add(form[4])
    DECODE_REACHED.add((S1_NAMES[form[0]], form[1], _vec_cause(case, form) if form[0] == 1 else "-", form[2], TK_NAMES[form[3]], case[8]))


def test_decode_rejects_a_workspace_below_its_alignment_and_writes_nothing():
    """The one pointer the launcher checks: the workspace at 8-byte alignment is CNL_E_BAD_ARG, from the launcher and from the query alike."""
    case = DECODE_CASES[0]
    heat_t, box_t, reid_t = _decode_data(case)
    heat, box, reid = StridedView(heat_t, "nhwc", "nan", "cuda"), StridedView(box_t, "nhwc", "nan", "cuda"), StridedView(reid_t, "nhwc", "nan", "cuda")
    outs, _, ws_bytes = _decode_outputs(case, "cuda")
    ws = GuardedBytes(ws_bytes, align=8, device="cuda", name="workspace at 8")
    p = _decode_params(case, heat, box, reid, outs, ws, ws_bytes)
    lib = _lib.load()
    assert lib.cnl_decode_forms(ctypes.byref(p), None, None, None, None) == _lib.CNL_E_BAD_ARG
    assert lib.cnl_decode_f32(ctypes.byref(p), _stream()) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
    p.workspace_bytes = ws_bytes - 1                                    # ... and one byte short of the promise
    ws16 = GuardedBytes(ws_bytes, align=16, device="cuda")
    p.workspace = ws16.ptr
    assert lib.cnl_decode_f32(ctypes.byref(p), _stream()) == _lib.CNL_E_WORKSPACE
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values()) and ws.untouched() and ws16.untouched()


@pytest.mark.parametrize("layouts", [("nchw_window_odd", "nhwc_ld3"), ("every_other_pixel_nhwc", "nchw_window"), ("batch_every_other", "batch_slice_nchw"),
                                     ("nhwc_wide", "nhwc_wide")], ids=lambda l: "-".join(l))
def test_standalone_gathers_of_strided_views_into_guarded_outputs(layouts):
    """cnl_gather_boxes_f32 / cnl_gather_embeddings_f32 at the reference's own indices (all four edges among them)."""
    N, C, H, W, k, E = 2, 3, 11, 14, 40, 5
    heat_t, box_t, reid_t = _decode_data(("gathers", N, C, H, W, k, 3, E, None, None, None, "ring", 4))
    ref = decode_ref.decode_detections(heat_t.numpy(), box_t.numpy(), k, 3, reid=reid_t.numpy())
    idx = ref["indices"]
    assert (idx // W == 0).any() and (idx // W == H - 1).any() and (idx % W == 0).any() and (idx % W == W - 1).any()
    lib = _lib.load()
    box, reid = StridedView(box_t, layouts[0], "nan", "cuda"), StridedView(reid_t, layouts[1], "nan", "cuda")
    indices = torch.from_numpy(idx).cuda()
    snap = indices.clone()
    boxes = GuardedBytes(N * k * 16, align=4, device="cuda", name="boxes")
    emb = GuardedBytes(N * k * E * 4, align=4, device="cuda", name="emb")
    assert lib.cnl_gather_boxes_f32(box.ptr, *box.strides, indices.data_ptr(), boxes.ptr, N, H, W, k, 0, 0, 1.0, 4.0, _stream()) == 0, _lib.last_error()
    assert lib.cnl_gather_embeddings_f32(reid.ptr, *reid.strides, indices.data_ptr(), emb.ptr, N, E, H, W, k, _stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(boxes)
    _ok(emb)
    assert box.unchanged() and reid.unchanged() and torch.equal(indices, snap)
    assert np.array_equal(_bits(boxes.result(torch.float32, (N, k, 4)).numpy()), _bits(ref["boxes"]))
    assert np.array_equal(_bits(emb.result(torch.float32, (N, k, E)).numpy()), _bits(ref["embeddings"]))


# ====================================================================================================================== collate and formats
def _guarded_input(a, align, name):
    """A numpy array as device bytes at exactly `align` inside NaN-pattern (0xFF) guards -> (GuardedBytes, snapshot of the whole allocation)."""
    a = np.ascontiguousarray(a)
    g = GuardedBytes(a.nbytes, align=align, device="cuda", sentinel=0xFF, name=name)
    g.body.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)))
    return g, g.alloc.clone()


@pytest.mark.parametrize("E", [0, 3, 64])
def test_pack_and_unpack_records_into_guarded_buffers(E):
    """cnl_pack_detections_f32 / cnl_unpack_detections_f32: element alignment everywhere, emb == NULL at E == 0, the round trip is the identity."""
    lib = _lib.load()
    N, k = 3, 37
    rng = np.random.default_rng(E)
    boxes, scores = rng.random((N, k, 4), dtype=np.float32) * 500, rng.random((N, k), dtype=np.float32)
    labels = rng.integers(-3, 90, (N, k)).astype(np.int64)
    emb = rng.standard_normal((N, k, E)).astype(np.float32) if E else None
    want = decode_ref.pack_detections(boxes, scores, labels, emb)
    ins = {"boxes": _guarded_input(boxes, 4, "boxes"), "scores": _guarded_input(scores, 4, "scores"), "labels": _guarded_input(labels, 8, "labels")}
    if E:
        ins["emb"] = _guarded_input(emb, 4, "emb")
    rec = GuardedBytes(N * k * (6 + E) * 4, align=4, device="cuda", name="rec")
    assert lib.cnl_pack_detections_f32(ins["boxes"][0].ptr, ins["scores"][0].ptr, ins["labels"][0].ptr, ins["emb"][0].ptr if E else None, rec.ptr,
                                       N, k, E, _stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(rec)
    assert all(torch.equal(g.alloc, snap) for g, snap in ins.values())
    assert np.array_equal(rec.result(torch.int32).numpy(), want.view(np.int32).reshape(-1))
    outs = {"boxes": GuardedBytes(boxes.nbytes, align=4, device="cuda", name="boxes out"), "scores": GuardedBytes(scores.nbytes, align=4, device="cuda", name="scores out"),
            "labels": GuardedBytes(labels.nbytes, align=8, device="cuda", name="labels out")}
    if E:
        outs["emb"] = GuardedBytes(emb.nbytes, align=4, device="cuda", name="emb out")
    snap = rec.alloc.clone()
    assert lib.cnl_unpack_detections_f32(rec.ptr, outs["boxes"].ptr, outs["scores"].ptr, outs["labels"].ptr, outs["emb"].ptr if E else None, N, k, E,
                                         _stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for g in outs.values():
        _ok(g)
    assert torch.equal(rec.alloc, snap)
    assert np.array_equal(outs["boxes"].result(torch.int32).numpy(), boxes.view(np.int32).reshape(-1))
    assert np.array_equal(outs["scores"].result(torch.int32).numpy(), scores.view(np.int32).reshape(-1))
    assert np.array_equal(outs["labels"].result(torch.int64).numpy(), labels.astype(np.int32).astype(np.int64).reshape(-1))
    if E:
        assert np.array_equal(outs["emb"].result(torch.int32).numpy(), emb.view(np.int32).reshape(-1))


def test_xyxy_to_xywh_out_of_place_in_place_and_below_its_alignment():
    """cnl_boxes_xyxy_to_xywh_f32 moves whole boxes: both pointers 16-byte aligned (stated in the header, checked by the launcher)."""
    lib = _lib.load()
    n = 301
    boxes = (np.random.default_rng(1).random((n, 4), dtype=np.float32) * 300).astype(np.float32)
    want = np.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], axis=1)
    src, snap = _guarded_input(boxes, 16, "boxes")
    out = GuardedBytes(n * 16, align=16, device="cuda", name="xywh")
    assert lib.cnl_boxes_xyxy_to_xywh_f32(src.ptr, out.ptr, n, _stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(out)
    assert torch.equal(src.alloc, snap) and np.array_equal(out.result(torch.int32).numpy(), want.view(np.int32).reshape(-1))
    assert lib.cnl_boxes_xyxy_to_xywh_f32(src.ptr, src.ptr, n, _stream()) == 0, _lib.last_error()         # in place
    torch.cuda.synchronize()
    assert np.array_equal(src.result(torch.int32).numpy(), want.view(np.int32).reshape(-1))
    snap[src.start:src.start + src.nbytes] = src.body
    assert torch.equal(src.alloc, snap)                                                                   # the guards of the in-place buffer
    low = GuardedBytes(n * 16, align=8, device="cuda", name="xywh at 8")
    assert lib.cnl_boxes_xyxy_to_xywh_f32(src.ptr, low.ptr, n, _stream()) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
    torch.cuda.synchronize()
    assert low.untouched()


# ====================================================================================================================== packed frames
FRAME_SIZES = [(50, 70), (7, 5), (1, 1), (97, 3), (33, 130), (64, 96), (2, 200), (31, 33)]
FILL = (114, 7, 201, 33)
PAD_BYTE = 255            # the row padding of the source frames; their pixels stay below 200, so no blend of pixels gives it


def _padded_frames(C, seed):
    """Frames with row_stride > w * C on the device: pixels in 0..199, row padding 255 -> ([numpy frames], [device buffers], [row strides])."""
    rng = np.random.default_rng(seed)
    host, dev, strides = [], [], []
    for i, (h, w) in enumerate(FRAME_SIZES):
        f = rng.integers(0, 200, (h, w, C), dtype=np.uint8)
        stride = w * C + 1 + (i % 3) * 5
        buf = np.full((h + 2, stride), PAD_BYTE, np.uint8)                    # one padding row before and after the frame as well
        buf[1:h + 1, :w * C] = f.reshape(h, w * C)
        host.append(f)
        dev.append(torch.from_numpy(buf).cuda())
        strides.append(stride)
    return host, dev, strides


def _letterbox_table(dev, strides, geo):
    recs = (_lib.LetterboxFrame * len(geo))()
    for i, (h, w, nh, nw, pt, pl) in enumerate(geo):
        recs[i].src = dev[i].data_ptr() + strides[i]                          # the frame's first pixel: behind the padding row
        recs[i].h, recs[i].w, recs[i].row_stride = h, w, strides[i]
        recs[i].new_h, recs[i].new_w, recs[i].pad_top, recs[i].pad_left = nh, nw, pt, pl
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("C", [1, 3, 4])
def test_letterbox_of_padded_frames_into_a_guarded_canvas(C):
    """cnl_letterbox_bilinear_u8: a mixed-size batch at a 64 x 96 canvas 4-byte aligned inside guards; every byte equals the oracle's, nothing else
    changes, the source rows' padding is never blended in; rejected arguments leave the canvas all sentinel."""
    lib = _lib.load()
    height, width = 64, 96
    host, dev, strides = _padded_frames(C, 40 + C)
    want, geo = letterbox_ref.expected_canvas(host, height, width, FILL)
    assert want.max() < PAD_BYTE                                              # (the fill is below 255 too)
    table = _letterbox_table(dev, strides, geo)
    snaps = [d.clone() for d in dev] + [table.clone()]
    N = len(host)
    fill = sum(FILL[c] << (8 * c) for c in range(4))
    for sentinel in (0xA5, 0x3C):
        out = GuardedBytes(N * height * width * C, align=4, device="cuda", sentinel=sentinel, name="canvas")
        assert lib.cnl_letterbox_bilinear_u8(table.data_ptr(), out.ptr, N, height, width, C, fill, _stream()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        _ok(out)
        got = out.result(torch.uint8, (N, height, width, C)).numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert all(torch.equal(a, b) for a, b in zip(dev + [table], snaps))
    out = GuardedBytes(N * height * width * C + 2, align=2, device="cuda", name="canvas at 2")
    for args in ((table.data_ptr(), out.ptr, N, height, width, C), (table.data_ptr(), out.ptr + 2, N, height, width, 5), (table.data_ptr(), out.ptr + 2, N, height, width + 8, C),
                 (table.data_ptr() + 4, out.ptr + 2, N, height, width, C)):
        assert lib.cnl_letterbox_bilinear_u8(*args, fill, _stream()) == _lib.CNL_E_BAD_ARG, args
    torch.cuda.synchronize()
    assert out.untouched()


def test_unletterbox_in_place_inside_guards():
    """cnl_unletterbox_boxes_f32: boxes at exactly 16-byte alignment, in place; the bound of test_gpu_letterbox.py; packed control bit for bit."""
    lib = _lib.load()
    host, dev, strides = _padded_frames(3, 9)
    _, geo = letterbox_ref.expected_canvas(host, 64, 96, FILL)
    table = _letterbox_table(dev, strides, geo)
    N, k = len(host), 23
    boxes = (np.random.default_rng(2).random((N, k, 4), dtype=np.float32) * np.float32([96, 64, 96, 64]) * 1.2 - 5).astype(np.float32)
    results = []
    for clip in (1, 0):
        g, snap = _guarded_input(boxes, 16, "boxes")
        assert lib.cnl_unletterbox_boxes_f32(g.ptr, table.data_ptr(), N, k, clip, _stream()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        got = g.result(torch.float32, (N, k, 4)).numpy()
        snap[g.start:g.start + g.nbytes] = g.body
        assert torch.equal(g.alloc, snap), "a byte outside the boxes changed"
        err = np.abs(got.astype(np.float64) - letterbox_ref.unletterbox_boxes(boxes, geo, clip=bool(clip)))
        assert (err <= letterbox_ref.unletterbox_bound(boxes, geo)).all(), np.argwhere(err > letterbox_ref.unletterbox_bound(boxes, geo))[:5].tolist()
        control = torch.from_numpy(boxes).cuda()                               # packed, allocation-aligned
        assert lib.cnl_unletterbox_boxes_f32(control.data_ptr(), table.data_ptr(), N, k, clip, _stream()) == 0
        assert np.array_equal(_bits(control.cpu().numpy()), _bits(got))
        results.append(got)
    assert not np.array_equal(results[0], results[1])                          # the clip bites on these boxes
    low, snap = _guarded_input(boxes, 8, "boxes at 8")
    assert lib.cnl_unletterbox_boxes_f32(low.ptr, table.data_ptr(), N, k, 1, _stream()) == _lib.CNL_E_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(low.alloc, snap)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize_normalize_and_mirror_into_guarded_outputs(C):
    """cnl_resize_bilinear_u8 (byte alignment), cnl_mirror_append_u8 (byte alignment: the dword form at 4, the byte form at 1) and, at C == 3,
    cnl_normalize_u8_nhwc_f32 (x at 4, y at 16: stated in the header, checked by the launcher)."""
    lib = _lib.load()
    rng = np.random.default_rng(70 + C)
    N, H, W = 2, 37, 53
    x = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    for align, (Ho, Wo) in ((1, (64, 96)), (4, (19, 31))):
        src, snap = _guarded_input(x, align, "x")
        y = GuardedBytes(N * Ho * Wo * C, align=align, device="cuda", name="resized")
        assert lib.cnl_resize_bilinear_u8(src.ptr, y.ptr, N, H, W, Ho, Wo, C, _stream()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        _ok(y)
        assert torch.equal(src.alloc, snap)
        assert np.array_equal(y.result(torch.uint8, (N, Ho, Wo, C)).numpy(), decode_ref.resize_bilinear_u8(x, Ho, Wo))
    for align, Wm in ((4, 52), (1, 52), (4, 53)):                              # row bytes % 4 == 0 at 4: dwords; otherwise bytes
        xm = np.ascontiguousarray(x[:, :, :Wm])
        src, snap = _guarded_input(xm, align, "x")
        dst = GuardedBytes(2 * xm.nbytes, align=align, device="cuda", name="mirrored")
        assert lib.cnl_mirror_append_u8(src.ptr, dst.ptr, N, H, Wm, C, _stream()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        _ok(dst)
        assert torch.equal(src.alloc, snap)
        assert np.array_equal(dst.result(torch.uint8, (2 * N, H, Wm, C)).numpy(), np.concatenate([xm, xm[:, :, ::-1]], axis=0))
    if C != 3:
        return
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    m255 = (ctypes.c_float * 3)(*(np.array(mean, np.float32) * np.float32(255)))
    inv = (ctypes.c_float * 3)(*np.reciprocal(np.array(std, np.float32) * np.float32(255), dtype=np.float32))
    for Wn in (53, 52):                                                        # pixels % 4 != 0: the scalar tail
        xn = np.ascontiguousarray(x[:, :, :Wn])
        src, snap = _guarded_input(xn, 4, "x")
        y = GuardedBytes(xn.size * 4, align=16, device="cuda", name="normalised")
        assert lib.cnl_normalize_u8_nhwc_f32(src.ptr, y.ptr, N, H, Wn, m255, inv, _stream()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        _ok(y)
        assert torch.equal(src.alloc, snap)
        assert np.array_equal(_bits(y.result(torch.float32, xn.shape).numpy()), _bits(decode_ref.normalize_u8(xn, mean, std)))
    low = GuardedBytes(x.size * 4, align=8, device="cuda", name="normalised at 8")
    src2 = GuardedBytes(x.nbytes, align=2, device="cuda", name="x at 2")
    assert lib.cnl_normalize_u8_nhwc_f32(src.ptr, low.ptr, N, H, W, m255, inv, _stream()) == _lib.CNL_E_BAD_ARG
    assert lib.cnl_normalize_u8_nhwc_f32(src2.ptr, y.ptr, N, H, W, m255, inv, _stream()) == _lib.CNL_E_BAD_ARG
    torch.cuda.synchronize()
    assert low.untouched()


# ====================================================================================================================== tile merge
def _merge_candidates(rng, records, ffv, k, n_objects):
    """Overlapping candidates in view pixels (the recipe of test_gpu_tiles.py, shortened): each frame's objects seen through each of its views."""
    V = len(records)
    boxes = np.zeros((V, k, 4), np.float32)
    for n in range(len(ffv) - 1):
        if ffv[n + 1] == ffv[n]:
            continue
        fw, fh = records[ffv[n]][0], records[ffv[n]][1]
        cx, cy, bw, bh = rng.uniform(0, fw, n_objects), rng.uniform(0, fh, n_objects), rng.uniform(20, 260, n_objects), rng.uniform(20, 260, n_objects)
        for v in range(ffv[n], ffv[n + 1]):
            _, _, x0, y0, pl, pt, sx, sy = records[v]
            o = rng.integers(0, n_objects, k)
            fb = np.stack([cx[o] - bw[o] / 2, cy[o] - bh[o] / 2, cx[o] + bw[o] / 2, cy[o] + bh[o] / 2], axis=1) + rng.uniform(-6, 6, (k, 4)) * (rng.random((k, 1)) < 0.7)
            boxes[v] = np.clip(np.stack([(fb[:, 0] - x0) * sx + pl, (fb[:, 1] - y0) * sy + pt, (fb[:, 2] - x0) * sx + pl, (fb[:, 3] - y0) * sy + pt], axis=1), -8, 520)
    scores = rng.choice(np.array([0.05, 0.15, 0.3, 0.5, 0.7, 0.9], np.float32), (V, k)).astype(np.float32)
    return boxes, scores, rng.integers(0, 3, (V, k)).astype(np.int64)


def _guarded_merge(boxes, scores, labels, records, ffv, K_out, cap, sentinel, out_boxes_align=16, ws_align=256, expect=0):
    lib = _lib.load()
    N, (V, k) = len(ffv) - 1, scores.shape
    geom = cl.TileGeometry.from_records(records, ffv, "cuda")
    ins = [_guarded_input(boxes, 16, "boxes"), _guarded_input(scores, 4, "scores"), _guarded_input(labels, 8, "labels")]
    tables = [geom.merge_table, geom.first_view]
    snaps = [t.clone() for t in tables]
    spec = {"bboxes": (K_out * 16, out_boxes_align), "scores": (K_out * 4, 4), "labels": (K_out * 8, 8), "source": (K_out * 4, 4), "count": (4, 4)}
    outs = {key: GuardedBytes(N * per, align=al, device="cuda", sentinel=sentinel, name=f"out_{key}") for key, (per, al) in spec.items()}
    ws_bytes = int(lib.cnl_merge_tiles_workspace_bytes(N, V, k, cap))
    assert ws_bytes > 0
    ws = GuardedBytes(ws_bytes, align=ws_align, device="cuda", sentinel=sentinel, name="merge workspace")
    rc = lib.cnl_merge_tiles_f32(ins[0][0].ptr, ins[1][0].ptr, ins[2][0].ptr, geom.merge_table.data_ptr(), geom.first_view.data_ptr(), N, V, k, K_out, cap, 0.1, 0.5, 0, 1,
                                 outs["bboxes"].ptr, outs["scores"].ptr, outs["labels"].ptr, outs["source"].ptr, outs["count"].ptr, ws.ptr, ws_bytes, _stream())
    assert rc == expect, _lib.last_error()
    torch.cuda.synchronize()
    if expect:
        assert all(g.untouched() for g in list(outs.values()) + [ws])
        return None
    for g in list(outs.values()) + [ws]:
        _ok(g)
    assert all(torch.equal(g.alloc, snap) for g, snap in ins) and all(torch.equal(a, b) for a, b in zip(tables, snaps))
    return {"bboxes": outs["bboxes"].result(torch.float32, (N, K_out, 4)).numpy(), "scores": outs["scores"].result(torch.float32, (N, K_out)).numpy(),
            "labels": outs["labels"].result(torch.int64, (N, K_out)).numpy(), "source": outs["source"].result(torch.int32, (N, K_out)).numpy(),
            "count": outs["count"].result(torch.int32, (N,)).numpy()}


def _merge_equal(got, want):
    for key in ("count", "source", "labels", "scores", "bboxes"):
        assert got[key].dtype == want[key].dtype and np.array_equal(_bits(got[key]), _bits(want[key])), (key, np.argwhere(got[key] != want[key])[:5].tolist())


@functools.lru_cache(maxsize=None)
def _merge_case(name):
    rng = np.random.default_rng(len(name))
    if name == "two_frames":                               # 2 x 5 views: K_out below and above the number kept
        rec, ffv, _ = tiled_ref.view_records([(700, 900), (300, 400)], 512, 512, 0.2, True, letterbox_ref.geometry)
        k, n_obj, cap = 40, 30, 4096
    elif name == "empty_frames":                           # frames without views between frames with
        rec, ffv, _ = tiled_ref.view_records([(300, 400)], 512, 512, 0.2, True, letterbox_ref.geometry)
        ffv, k, n_obj, cap = [0, 0, len(rec), len(rec)], 25, 10, 64
    elif name == "no_views":                               # V == 0
        rec, ffv, k, n_obj, cap = [], [0, 0, 0], 8, 1, 16
    else:                                                  # "large": 61 views x 100: the frame leaves the LDS sort (6000 candidates pass, the sort pads to 8192 keys)
        rec, ffv, _ = tiled_ref.view_records([(2160, 3840)], 512, 512, 0.2, True, letterbox_ref.geometry)
        k, n_obj, cap = 100, 400, 8192
    boxes, scores, labels = _merge_candidates(rng, rec, ffv, k, n_obj)
    if name == "large":
        scores[scores < 0.1] = 0.15
        scores.reshape(-1)[rng.choice(scores.size, 100, replace=False)] = 0.05
        assert len(rec) == 61 and (scores > np.float32(0.1)).sum() == 6000
    return boxes, scores, labels, rec, ffv, cap


@pytest.mark.parametrize("name,K_out", [("two_frames", 7), ("two_frames", 300), ("empty_frames", 50), ("no_views", 5), ("large", 300)])
def test_tile_merge_into_five_guarded_outputs(name, K_out):
    """cnl_merge_tiles_f32: outputs at their stated alignment (out_boxes 16, the rest their element's), the workspace exactly the promised size at exactly
    256; "every output element is written" = equality with tests/tiled_ref.merge_ref under two different sentinel bytes."""
    boxes, scores, labels, rec, ffv, cap = _merge_case(name)
    want = tiled_ref.merge_ref(boxes, scores, labels, rec, ffv, K_out, max_candidates=cap)
    if name == "two_frames":
        assert (want["count"] == 7).all() if K_out == 7 else (0 < want["count"]).all() and (want["count"] < K_out).all()
    for sentinel in (0xA5, 0x3C):
        _merge_equal(_guarded_merge(boxes, scores, labels, rec, ffv, K_out, cap, sentinel), want)
    if name == "two_frames":                               # the pointers the launcher checks, below their alignment: refused, nothing written
        _guarded_merge(boxes, scores, labels, rec, ffv, K_out, cap, 0xA5, out_boxes_align=8, expect=_lib.CNL_E_BAD_ARG)
        _guarded_merge(boxes, scores, labels, rec, ffv, K_out, cap, 0xA5, ws_align=128, expect=_lib.CNL_E_WORKSPACE)


# ====================================================================================================================== COCO
@pytest.mark.parametrize("name", ["small", "over64", "empty"])
def test_coco_match_and_accumulate_into_guarded_outputs(name):
    """cnl_coco_match_f64 / cnl_coco_accumulate_f64 on the cases of test_gpu_coco_eval.py: NaN boxes and scores in the slots past count, NaN ground truths
    past gt_count, npig incremented from a nonzero start; ranks, masks, npig, precision and recall equal tests/coco_eval_ref.py (float64 bits)."""
    import test_gpu_coco_eval as coco_t
    lib = _lib.load()
    boxes, scores, labels, count, gts, K = coco_t.case(name)
    want = coco_t.expected(name, True)
    N, k = scores.shape
    boxes, scores = boxes.copy(), scores.copy()
    for n in range(N):
        boxes[n, count[n]:], scores[n, count[n]:] = np.nan, np.nan
    Gmax = max(len(l) for _, l in gts) + 3
    gt_boxes, gt_labels = np.full((N, Gmax, 4), np.nan), np.full((N, Gmax), 1, np.int64)
    for n, (b, l) in enumerate(gts):
        gt_boxes[n, :len(l)], gt_labels[n, :len(l)] = b, l
    gt_count = np.array([len(l) for _, l in gts], np.int32)
    ins = [_guarded_input(boxes, 16, "boxes"), _guarded_input(scores, 4, "scores"), _guarded_input(labels, 8, "labels"), _guarded_input(count, 4, "count"),
           _guarded_input(gt_boxes, 8, "gt_boxes"), _guarded_input(gt_labels, 8, "gt_labels"), _guarded_input(gt_count, 4, "gt_count")]
    rank = GuardedBytes(N * k * 4, align=4, device="cuda", name="out_rank")
    matched, ignored = GuardedBytes(N * k * 8, align=8, device="cuda", name="out_matched"), GuardedBytes(N * k * 8, align=8, device="cuda", name="out_ignored")
    npig = GuardedBytes(K * 4 * 8, align=8, device="cuda", name="npig")
    start = torch.arange(1000, 1000 + K * 4, dtype=torch.int64)
    npig.typed(torch.int64).copy_(start)
    assert lib.cnl_coco_match_f64(*(g.ptr for g, _ in ins), N, k, Gmax, K, rank.ptr, matched.ptr, ignored.ptr, npig.ptr, _stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for g in (rank, matched, ignored, npig):
        _ok(g)
    assert all(torch.equal(g.alloc, snap) for g, snap in ins)
    assert np.array_equal((npig.result(torch.int64) - start).numpy().reshape(K, 4), want["npig"])
    r, m, i = rank.result(torch.int32, (N, k)).numpy(), matched.result(torch.int64, (N, k)).numpy(), ignored.result(torch.int64, (N, k)).numpy()
    for n in range(N):
        c = count[n]
        _, _, wr, wm, wi = want["records"][n]
        assert np.array_equal(r[n, :c], wr) and np.array_equal(m[n, :c], wm) and np.array_equal(i[n, :c], wi), n
        assert (r[n, c:] == -1).all() and (m[n, c:] == 0).all() and (i[n, c:] == 0).all()
    low, _ = _guarded_input(boxes, 8, "boxes at 8")        # boxes below their 16 bytes: refused, nothing written
    fresh = [GuardedBytes(N * k * 4, align=4, device="cuda"), GuardedBytes(N * k * 8, align=8, device="cuda"), GuardedBytes(N * k * 8, align=8, device="cuda"),
             GuardedBytes(K * 4 * 8, align=8, device="cuda")]
    assert lib.cnl_coco_match_f64(low.ptr, *(g.ptr for g, _ in ins[1:]), N, k, Gmax, K, *(g.ptr for g in fresh), _stream()) == _lib.CNL_E_BAD_ARG
    torch.cuda.synchronize()
    assert all(g.untouched() for g in fresh)
    # the epoch's records in the accumulate's order: by category, inside it by descending score, stably; dropped records last
    total = N * k
    rank_d, matched_d, ignored_d = rank.typed(torch.int32), matched.typed(torch.int64), ignored.typed(torch.int64)
    score_d, label_d = torch.from_numpy(np.nan_to_num(scores, nan=0.0).reshape(-1)).cuda(), torch.from_numpy(labels.reshape(-1)).cuda()
    by_score = torch.sort(score_d + 0.0, descending=True, stable=True).indices
    category, by_category = torch.sort(torch.where(rank_d >= 0, label_d, K)[by_score], stable=True)
    order = by_score[by_category]
    first = torch.searchsorted(category, torch.arange(K + 1, device="cuda", dtype=torch.int64)).contiguous()
    acc_in = [_guarded_input(rank_d[order].cpu().numpy(), 4, "rank"), _guarded_input(matched_d[order].cpu().numpy(), 8, "matched"),
              _guarded_input(ignored_d[order].cpu().numpy(), 8, "ignored"), _guarded_input(first.cpu().numpy(), 8, "segment_first")]
    npig_in, npig_snap = _guarded_input(want["npig"].astype(np.int64), 8, "npig")
    precision = GuardedBytes(want["precision"].nbytes, align=8, device="cuda", name="precision")
    recall = GuardedBytes(want["recall"].nbytes, align=8, device="cuda", name="recall")
    assert lib.cnl_coco_accumulate_f64(*(g.ptr for g, _ in acc_in), npig_in.ptr, total, K, precision.ptr, recall.ptr, _stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(precision)
    _ok(recall)
    assert all(torch.equal(g.alloc, snap) for g, snap in acc_in) and torch.equal(npig_in.alloc, npig_snap)
    assert np.array_equal(precision.result(torch.int64).numpy(), want["precision"].view(np.int64).reshape(-1))      # every element written: none keeps the sentinel
    assert np.array_equal(recall.result(torch.int64).numpy(), want["recall"].view(np.int64).reshape(-1))


# ====================================================================================================================== tracker
METRIC_NAMES = {0: "cosine", 1: "euclidean", 6: "braycurtis", 7: "correlation"}


class _FloatIn:
    """A float32 input inside an allocation of `fill` (NaN, +inf): the body 16-byte aligned, or `off` floats behind that."""

    def __init__(self, a, fill=float("nan"), off=0):
        a = np.ascontiguousarray(a, np.float32)
        self.alloc = torch.full((2048 + a.size + off,), fill, dtype=torch.float32, device="cuda")
        self.alloc[1024 + off:1024 + off + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        self.ptr = self.alloc.data_ptr() + 4 * (1024 + off)
        self.snapshot = self.alloc.clone()

    def unchanged(self):
        return bool((self.alloc.view(torch.int32) == self.snapshot.view(torch.int32)).all())


def _track_data(k, T, E, seed):
    """Detections and a track table whose rows are noisy copies of some detections (so that both assignment stages find pairs)."""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((k, E)).astype(np.float32)
    c, sz = rng.random((k, 2)), rng.random((k, 2)) * 0.3 + 0.05
    dbox = np.concatenate([c - sz / 2, c + sz / 2], 1).astype(np.float32)
    src = rng.permutation(k)[:T]
    temb = (emb[src] + 0.15 * rng.standard_normal((T, E))).astype(np.float32)
    temb[1::3] = rng.standard_normal((len(temb[1::3]), E)).astype(np.float32)        # a third of the tracks match through their boxes only
    tbox = (dbox[src] + 0.01 * rng.standard_normal((T, 4))).astype(np.float32)
    score = rng.random(k).astype(np.float32)
    score[rng.integers(0, k)] = np.float32(0.3)                                      # exactly at the threshold: kept
    return emb, temb, dbox, tbox, score


def _plain_costs(emb, dbox, score, temb, tbox, box_cost, metric):
    """cnl_track_costs_metric_f32 on packed tensors: the separate buffers the record forms are compared with."""
    lib = _lib.load()
    k, E = emb.shape
    T = temb.shape[0]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    de, db, ds, te, tb = d(emb), d(dbox), d(score), d(temb), d(tbox)
    n_det, idx = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(k, dtype=torch.int32, device="cuda")
    reid, box = torch.zeros(max(k * T, 1), dtype=torch.float64, device="cuda"), torch.zeros(max(k * T, 1), dtype=torch.float32, device="cuda")
    rc = lib.cnl_track_costs_metric_f32(de.data_ptr(), db.data_ptr(), ds.data_ptr(), k, E, 0.3, te.data_ptr() if T else None, tb.data_ptr() if T else None, T, box_cost,
                                        metric, n_det.data_ptr(), idx.data_ptr(), reid.data_ptr(), box.data_ptr(), _stream())
    assert rc == 0, _lib.last_error()
    n = int(n_det.item())
    return n, idx.cpu().numpy()[:n], reid.cpu().numpy()[:n * T].reshape(n, T), box.cpu().numpy()[:n * T].reshape(n, T)


@pytest.mark.parametrize("E", [5, 64, 129])
@pytest.mark.parametrize("metric", [0, 1, 6, 7])
def test_track_costs_write_only_the_n_by_T_part(metric, E):
    """cnl_track_costs_metric_f32: det_index[k], reid_cost[k * T] and box_cost_out[k * T] are sized for n = k; with 0 < n < k only the first n indices and
    the n x T parts change.  Embeddings and boxes sit in NaN, the scores in +inf (a score read past k would be kept).  Bars of test_gpu_tracker.py."""
    from scipy.spatial.distance import cdist
    lib = _lib.load()
    k, T = 40, 13
    emb, temb, dbox, tbox, score = _track_data(k, T, E, 100 * metric + E)
    keep = score >= np.float32(0.3)
    n = int(keep.sum())
    assert 0 < n < k
    off = 0 if E % 4 == 0 else 1                            # the embeddings at exactly their stated alignment: 16 bytes when E % 4 == 0, else 4
    for box_cost, TT in ((1, T), (0, T), (2, T), (1, 0)):
        ins = [_FloatIn(emb, off=off), _FloatIn(dbox), _FloatIn(score, float("inf")), _FloatIn(temb[:TT], off=off), _FloatIn(tbox[:TT])]
        n_det = GuardedBytes(4, align=4, device="cuda", name="n_det")
        det_index = GuardedBytes(4 * k, align=4, device="cuda", mask=record_mask(1, 4 * k, 4 * n), name="det_index")
        reid = GuardedBytes(8 * k * TT, align=8, device="cuda", mask=record_mask(1, 8 * k * TT, 8 * n * TT), name="reid_cost")
        box = GuardedBytes(4 * k * TT, align=4, device="cuda", mask=record_mask(1, 4 * k * TT, 4 * n * TT if box_cost else 0), name="box_cost_out")
        rc = lib.cnl_track_costs_metric_f32(ins[0].ptr, ins[1].ptr, ins[2].ptr, k, E, 0.3, ins[3].ptr if TT else None, ins[4].ptr if TT else None, TT, box_cost, metric,
                                            n_det.ptr, det_index.ptr, reid.ptr, box.ptr, _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        for g in (n_det, det_index, reid, box):
            _ok(g)
        assert all(i.unchanged() for i in ins)
        if not box_cost:
            assert box.untouched()
        assert int(n_det.result(torch.int32)) == n and np.array_equal(det_index.result(torch.int32).numpy()[:n], np.nonzero(keep)[0])
        if not TT:
            continue
        got, want = reid.result(torch.float64).numpy()[:n * TT].reshape(n, TT), cdist(emb[keep], temb, METRIC_NAMES[metric])
        if metric in (0, 7):
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        else:
            assert np.array_equal(got, want)
        if box_cost:
            ref = (tracker_ref.box_iou_distance_matrix if box_cost == 1 else tracker_ref.box_giou_distance_matrix)(dbox[keep], tbox)
            assert np.array_equal(_bits(box.result(torch.float32).numpy()[:n * TT].reshape(n, TT)), _bits(ref.astype(np.float32)))
        if box_cost == 1:                                   # (d): the packed control
            pn, pidx, preid, pbox = _plain_costs(emb, dbox, score, temb, tbox, 1, metric)
            assert pn == n and np.array_equal(preid.view(np.int64), got.view(np.int64)) and np.array_equal(_bits(pbox), _bits(box.result(torch.float32).numpy()[:n * TT].reshape(n, TT)))


def test_track_costs_refuse_inputs_below_their_alignment():
    lib = _lib.load()
    k, T, E = 40, 13, 64
    emb, temb, dbox, tbox, score = _track_data(k, T, E, 5)
    outs = [GuardedBytes(4, align=4, device="cuda"), GuardedBytes(4 * k, align=4, device="cuda"), GuardedBytes(8 * k * T, align=8, device="cuda"),
            GuardedBytes(4 * k * T, align=4, device="cuda")]
    for which in range(4):                                   # det_emb, det_box, trk_emb, trk_box in turn, 4 bytes off
        ins = [_FloatIn(emb, off=which == 0), _FloatIn(dbox, off=which == 1), _FloatIn(score), _FloatIn(temb, off=which == 2), _FloatIn(tbox, off=which == 3)]
        rc = lib.cnl_track_costs_metric_f32(ins[0].ptr, ins[1].ptr, ins[2].ptr, k, E, 0.3, ins[3].ptr, ins[4].ptr, T, 1, 0, *(g.ptr for g in outs), _stream())
        assert rc == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error(), which
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)


def test_tracker_host_path_copies_views_that_start_off_a_16_byte_boundary():
    """Tracker.update / TrackerBank hand their detections through _to_dev: a contiguous device view 4 bytes into a buffer reaches the launchers aligned."""
    flat = torch.arange(1 + 40 * 4, dtype=torch.float32, device="cuda")
    view, whole = flat[1:].reshape(40, 4), flat[4:160].reshape(39, 4)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and whole.data_ptr() % 16 == 0
    got = _track_host._to_dev(view, view.device)
    assert got.data_ptr() % 16 == 0 and torch.equal(got, view) and _track_host._to_dev(whole, whole.device) is whole


def _frame_mask(h, need, with_box):
    """The bytes of a frame record the kernel may write, from the record's own header: header, n indices, the detections, the n x T matrices."""
    hdr = h[:32].view(np.int32).tolist()
    n, k, T, with_dets, off_index, off_dets, off_reid, off_box = hdr
    m = torch.zeros(need, dtype=torch.bool)
    m[:32] = True
    m[off_index:off_index + 4 * n] = True
    if with_dets:
        m[off_dets:off_dets + 24 * k] = True
    m[off_reid:off_reid + 8 * n * T] = True
    if with_box:
        m[off_box:off_box + 4 * n * T] = True
    return m


@pytest.mark.parametrize("where", ["device", "mapped_host"])
@pytest.mark.parametrize("T", [13, 0])
def test_track_frame_record_of_exactly_the_promised_bytes(T, where):
    """cnl_track_frame_f32 into a record of exactly cnl_track_frame_bytes at exactly 8-byte alignment, in device memory and inside a larger block of
    cnl_host_alloc memory; with and without detections, every label kind; equal to the separate buffers of cnl_track_costs_metric_f32 bit for bit."""
    lib = _lib.load()
    k, E, box_cost, metric = 40, 64, 1, 0
    emb, temb, dbox, tbox, score = _track_data(k, 13, E, 77)
    temb, tbox = temb[:T], tbox[:T]
    labels = np.random.default_rng(1).integers(0, 80, k)
    n, idx, reid, box = _plain_costs(emb, dbox, score, temb, tbox, box_cost, metric)
    assert 0 < n < k
    ins = [_FloatIn(emb), _FloatIn(dbox), _FloatIn(score, float("inf")), _FloatIn(temb), _FloatIn(tbox)]
    for with_dets, kind, dtype in ((0, 0, None), (1, 1, np.int64), (1, 2, np.int32), (1, 3, np.float32)):
        lab = torch.from_numpy(labels.astype(dtype)).cuda() if kind else None
        need = int(lib.cnl_track_frame_bytes(k, T, with_dets))
        block = ctypes.c_void_p()
        if where == "mapped_host":
            total = GuardedBytes.wrapped_bytes(need, align=8)
            _lib.check(lib.cnl_host_alloc(total, ctypes.byref(block)), "cnl_host_alloc")
            rec = GuardedBytes(need, align=8, wrap=(block.value, total), name="record (mapped host)")
        else:
            rec = GuardedBytes(need, align=8, device="cuda", name="record (device)")
        try:
            rc = lib.cnl_track_frame_f32(ins[0].ptr, ins[1].ptr, ins[2].ptr, lab.data_ptr() if kind else None, kind, k, E, 0.3, ins[3].ptr if T else None,
                                         ins[4].ptr if T else None, T, box_cost, metric, with_dets, rec.ptr, need, _stream())
            assert rc == 0, _lib.last_error()
            torch.cuda.synchronize()
            h = rec.body.cpu().numpy().copy()
            _ok(rec, _frame_mask(h, need, box_cost))
        finally:
            del rec
            if where == "mapped_host":
                _lib.check(lib.cnl_host_free(block), "cnl_host_free")
        gn, gidx, gbox, gscore, glab, greid, gcost = _track_host.read_frame_record(h, True)
        assert gn == n and np.array_equal(gidx, idx) and h[:32].view(np.int32).tolist()[:4] == [n, k, T, with_dets]
        assert np.array_equal(greid.view(np.int64), reid.view(np.int64)) and np.array_equal(_bits(np.ascontiguousarray(gcost)), _bits(box))
        if with_dets:
            assert np.array_equal(_bits(gbox), _bits(dbox)) and np.array_equal(_bits(np.ascontiguousarray(gscore)), _bits(score)) and np.array_equal(glab, labels)
    assert all(i.unchanged() for i in ins)
    # what the launcher checks, below its alignment: the record at 4 bytes and (with tracks) det_box / trk_emb 4 bytes off -> refused, nothing written
    need = int(lib.cnl_track_frame_bytes(k, T, 0))
    rec4, rec8 = GuardedBytes(need, align=4, device="cuda", name="record at 4"), GuardedBytes(need, align=8, device="cuda", name="record")
    off_box, off_emb = _FloatIn(dbox, off=1), _FloatIn(temb, off=1)
    call = lambda de, db, te, rec: lib.cnl_track_frame_f32(de, db, ins[2].ptr, None, 0, k, E, 0.3, te if T else None, ins[4].ptr if T else None, T, box_cost, metric, 0,
                                                          rec.ptr, need, _stream())
    assert call(ins[0].ptr, ins[1].ptr, ins[3].ptr, rec4) == _lib.CNL_E_BAD_ARG and "8-byte" in _lib.last_error()
    if T:
        assert call(ins[0].ptr, off_box.ptr, ins[3].ptr, rec8) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
        assert call(ins[0].ptr, ins[1].ptr, off_emb.ptr, rec8) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
    else:                                                   # without tracks nothing is read 16 bytes at a time: the same pointer is accepted
        assert call(ins[0].ptr, off_box.ptr, None, rec8) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert rec4.untouched() and rec8.untouched() == bool(T)


@pytest.mark.parametrize("E", [1, 63, 65, 300])
def test_track_apply_into_guarded_tables(E):
    """cnl_track_apply_f32: rows of all three kinds into new_emb [T_new, E] / new_box at 4-byte alignment; the bars of test_gpu_tracker.py's test_apply_kernel."""
    lib = _lib.load()
    rng = np.random.default_rng(E)
    T, k, s = 9, 20, 0.3
    old_e, old_b = rng.standard_normal((T, E)).astype(np.float32), rng.random((T, 4)).astype(np.float32)
    det_e, det_b = rng.standard_normal((k, E)).astype(np.float32), rng.random((k, 4)).astype(np.float32)
    src_trk, src_det = np.array([0, 2, 3, -1, 8, -1, 5], np.int32), np.array([-1, 4, -1, 7, 19, 0, -1], np.int32)
    T_new = len(src_trk)
    ins = [_FloatIn(old_e, off=1), _FloatIn(old_b, off=1), _FloatIn(det_e, off=1), _FloatIn(det_b, off=1)]
    st, sd = torch.from_numpy(src_trk).cuda(), torch.from_numpy(src_det).cuda()
    new_emb, new_box = GuardedBytes(T_new * E * 4, align=4, device="cuda", name="new_emb"), GuardedBytes(T_new * 16, align=4, device="cuda", name="new_box")
    rc = lib.cnl_track_apply_f32(*(i.ptr for i in ins), st.data_ptr(), sd.data_ptr(), T_new, E, s, new_emb.ptr, new_box.ptr, _stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(new_emb)
    _ok(new_box)
    assert all(i.unchanged() for i in ins) and np.array_equal(st.cpu().numpy(), src_trk) and np.array_equal(sd.cpu().numpy(), src_det)
    ne, nb = new_emb.result(torch.float32, (T_new, E)).numpy(), new_box.result(torch.float32, (T_new, 4)).numpy()
    for r, (t, dd) in enumerate(zip(src_trk, src_det)):
        if dd < 0:
            assert np.array_equal(_bits(ne[r]), _bits(old_e[t])) and np.array_equal(_bits(nb[r]), _bits(old_b[t]))
            continue
        unit = det_e[dd] / np.linalg.norm(det_e[dd])
        np.testing.assert_allclose(ne[r], unit if t < 0 else (1 - s) * old_e[t] + s * unit, rtol=0, atol=2e-7)
        assert np.array_equal(_bits(nb[r]), _bits(det_b[dd]))


# ====================================================================================================================== assignment and streams
def test_lsap_segments_with_sentinel_gaps():
    """cnl_lsap_batch_f64: col4row segments 64 int32 apart inside one guarded buffer; row_stride > n_cols with NaN in the padding columns; problems with
    status 1, 2, 3 write nothing; rows > cols leave -1.  Equal to tests/lsap_ref.py (the restatement of scipy's algorithm)."""
    lib = _lib.load()
    rng = np.random.default_rng(12)
    shapes = [(12, 20), (20, 12), (7, 7), (1, 30), (15, 9), (9, 15), (40, 3), (33, 41)]
    mats = [lsap_ref.matrices(lsap_ref.KINDS[b % 4], n, T, rng) for b, (n, T) in enumerate(shapes)]
    mats[2][3, 4] = np.nan                                   # status 1
    mats[4][:, 2] = np.inf                                   # status 2: 15 x 9, every column must be assigned, this one cannot
    want_status = [0, 0, 1, 0, 2, 0, 0, 3]                   # the last lies beyond max_rows x max_cols = 40 x 30
    pad, seg = 3, 64
    flat, offs, o = [], [], 0
    for m in mats:
        buf = np.full((m.shape[0], m.shape[1] + pad), np.nan)
        buf[:, :m.shape[1]] = m
        flat.append(buf.ravel())
        offs.append(o)
        o += buf.size
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(np.asarray(a, t))).cuda()
    cost, cost_snap = _guarded_input(np.concatenate(flat), 8, "cost")
    c_off, o_off = d(offs, np.int64), d([b * seg for b in range(len(mats))], np.int64)
    ld, nr, nc = d([m.shape[1] + pad for m in mats], np.int32), d([m.shape[0] for m in mats], np.int32), d([m.shape[1] for m in mats], np.int32)
    col = GuardedBytes(len(mats) * seg * 4, align=4, device="cuda", name="col4row",
                       mask=record_mask(len(mats), seg * 4, [4 * m.shape[0] if st == 0 else 0 for m, st in zip(mats, want_status)]))
    status = GuardedBytes(len(mats) * 4, align=4, device="cuda", name="status")
    rc = lib.cnl_lsap_batch_f64(cost.ptr, c_off.data_ptr(), ld.data_ptr(), nr.data_ptr(), nc.data_ptr(), len(mats), 40, 30, col.ptr, o_off.data_ptr(), status.ptr, _stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(col)
    _ok(status)
    assert torch.equal(cost.alloc, cost_snap)
    assert status.result(torch.int32).tolist() == want_status
    got = col.result(torch.int32, (len(mats), seg)).numpy()
    for b, m in enumerate(mats):
        if want_status[b]:
            continue
        rows, cols = lsap_ref.linear_sum_assignment(m)
        want = np.full(m.shape[0], -1, np.int32)
        want[rows] = cols
        assert np.array_equal(got[b, :m.shape[0]], want), b
    assert (got[6, :40] == -1).sum() == 37                   # 40 x 3: rows > cols


def _stream_mask(r, stride):
    """The bytes of one live stream's record the kernels may write, from the record's own header."""
    hdr = r[:64].view(np.int32).tolist()
    S = _track_host
    m = torch.zeros(stride, dtype=torch.bool)
    m[:64] = True
    m[hdr[S.S_OFF_INDEX]:hdr[S.S_OFF_INDEX] + 4 * hdr[S.S_N]] = True
    if hdr[S.S_WITH_DETS]:
        m[hdr[S.S_OFF_DETS]:hdr[S.S_OFF_DETS] + 24 * hdr[S.S_K]] = True
    m[hdr[S.S_OFF_MATCH]:hdr[S.S_OFF_MATCH] + 8 * hdr[S.S_M]] = True
    m[hdr[S.S_OFF_UDET]:hdr[S.S_OFF_UDET] + 4 * hdr[S.S_NUDET]] = True
    m[hdr[S.S_OFF_UTRK]:hdr[S.S_OFF_UTRK] + 4 * hdr[S.S_NUTRK]] = True
    return m


def test_track_streams_workspace_records_and_gaps():
    """cnl_track_streams_f32: a workspace of exactly cnl_track_streams_workspace_bytes, record_stride larger than cnl_track_streams_record_bytes with the
    gaps and the records of the streams not in `live` left alone, R < S * T_max, a stream without tracks and one without detections.  The lists equal the
    single-stream path's (cnl_track_frame_f32 + the host's two-stage assignment), stage 1 also tests/lsap_ref.py's."""
    lib = _lib.load()
    S, live, k, E = 5, [3, 0, 4], 24, 64
    T_of = [6, 9, 4, 0, 11]                                  # stream 3 has no tracks; streams 1 and 2 take no part
    trk_off = np.concatenate([[0], np.cumsum(T_of)]).astype(np.int32)
    R, T_max = int(trk_off[-1]), 11
    assert R < S * T_max
    reid_thr, box_thr, box_cost, metric = 0.2, 0.5, 1, 0
    per = [_track_data(k, T_of[s], E, 300 + s) for s in live]
    per[1][4][:] = np.float32(0.1)                           # slot 1 (stream 0): no detection reaches the threshold
    det_emb, det_box, det_score = (np.stack([p[j] for p in per]) for j in (0, 2, 4))
    det_label = np.random.default_rng(3).integers(0, 80, (len(live), k)).astype(np.int64)
    pool_e, pool_b = np.random.default_rng(4).standard_normal((R, E)).astype(np.float32), np.random.default_rng(5).random((R, 4)).astype(np.float32)
    for i, s in enumerate(live):
        pool_e[trk_off[s]:trk_off[s + 1]], pool_b[trk_off[s]:trk_off[s + 1]] = per[i][1], per[i][3]
    ins = [_FloatIn(det_emb), _FloatIn(det_box), _FloatIn(det_score, float("inf")), _FloatIn(pool_e), _FloatIn(pool_b)]
    lab, live_d, off_d = torch.from_numpy(det_label).cuda(), torch.tensor(live, dtype=torch.int32).cuda(), torch.from_numpy(trk_off).cuda()
    ws_bytes = int(lib.cnl_track_streams_workspace_bytes(S, k, T_max))
    rec_bytes = int(lib.cnl_track_streams_record_bytes(k, T_max, 1))
    stride = rec_bytes + 40
    assert ws_bytes > 0 and rec_bytes > 0 and stride % 8 == 0
    ws = GuardedBytes(ws_bytes, align=8, device="cuda", name="streams workspace")
    rec = GuardedBytes(S * stride, align=8, device="cuda", name="stream records")
    rc = lib.cnl_track_streams_f32(ins[0].ptr, ins[1].ptr, ins[2].ptr, lab.data_ptr(), 1, S, len(live), live_d.data_ptr(), k, E, 0.3, reid_thr, box_thr, ins[3].ptr, ins[4].ptr,
                                   off_d.data_ptr(), R, T_max, box_cost, metric, 1, ws.ptr, ws_bytes, rec.ptr, stride, _stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(ws)
    h = rec.body.cpu().numpy().copy()
    mask = torch.zeros(S * stride, dtype=torch.bool)
    for s in live:
        mask[s * stride:(s + 1) * stride] = _stream_mask(h[s * stride:(s + 1) * stride], stride)
        assert not mask[s * stride + rec_bytes:(s + 1) * stride].any()
    _ok(rec, mask)
    assert all(i.unchanged() for i in ins)
    seen_empty = set()
    for i, s in enumerate(live):
        emb, temb, dbox, tbox, score = per[i]
        n, idx, reid, box = _plain_costs(emb, dbox, score, temb, tbox, box_cost, metric)
        want = _track_host.two_stage_assignment(reid, reid_thr, box_thr, box) if n else ([], [], list(range(T_of[s])))
        gn, gT, status, gidx, gbox, gscore, glab, matches, udet, utrk = _track_host.read_stream_record(h[s * stride:(s + 1) * stride])
        assert (gn, gT, status) == (n, T_of[s], 0) and np.array_equal(gidx, idx), (s, gn, gT, status)
        assert matches == [tuple(int(v) for v in p) for p in want[0]] and udet == list(want[1]) and utrk == list(want[2]), s
        assert np.array_equal(_bits(gbox), _bits(dbox)) and np.array_equal(glab, det_label[i])
        hdr = h[s * stride:s * stride + 64].view(np.int32)
        assert hdr[_track_host.S_SLOT] == i and hdr[_track_host.S_STREAM] == s
        if n and T_of[s]:
            rows, cols = lsap_ref.linear_sum_assignment(reid)
            stage1 = [(int(r), int(c)) for r, c in zip(rows, cols) if reid[r, c] < reid_thr]
            assert matches[:hdr[_track_host.S_M1]] == stage1 and 0 < len(stage1) < len(matches), (s, len(stage1), len(matches))
        seen_empty |= {"n == 0"} if n == 0 else set()
        seen_empty |= {"T == 0"} if T_of[s] == 0 else set()
    assert seen_empty == {"n == 0", "T == 0"}
    rec4 = GuardedBytes(S * stride, align=4, device="cuda", name="stream records at 4")      # record / workspace below 8 bytes: refused, nothing written
    ws.refill()
    args = (ins[0].ptr, ins[1].ptr, ins[2].ptr, lab.data_ptr(), 1, S, len(live), live_d.data_ptr(), k, E, 0.3, reid_thr, box_thr, ins[3].ptr, ins[4].ptr, off_d.data_ptr(), R, T_max,
            box_cost, metric, 1)
    assert lib.cnl_track_streams_f32(*args, ws.ptr, ws_bytes, rec4.ptr, stride, _stream()) == _lib.CNL_E_BAD_ARG
    assert lib.cnl_track_streams_f32(*args, ws.ptr + 4, ws_bytes - 4, rec.ptr, stride, _stream()) == _lib.CNL_E_BAD_ARG
    rec.refill()                                             # ... and det_box / trk_emb 4 bytes off
    off_box, off_emb = _FloatIn(det_box, off=1), _FloatIn(pool_e, off=1)
    for a in ((ins[0].ptr, off_box.ptr) + args[2:], args[:13] + (off_emb.ptr,) + args[14:]):
        assert lib.cnl_track_streams_f32(*a, ws.ptr, ws_bytes, rec.ptr, stride, _stream()) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
    torch.cuda.synchronize()
    assert rec4.untouched() and ws.untouched() and rec.untouched()


# ====================================================================================================================== coverage (keep last)
DECODE_REQUIRED = [
    # every stage-1 kernel; both strip heights of the C % 8 == 0 one
    ("c8", 4, "-", 4), ("c8", 4, "-", 16),
    # the channel-minor kernel at 4 / 2 / 1 floats per load, through C (C = 12 / 6 / 5 in a layout that allows 4) ...
    ("cminor", 4, "C", 8), ("cminor", 2, "C", 8), ("cminor", 1, "C", 8),
    # ... and, below 4, through a stride or the base pointer of a C that allows 4 (ok(4) / ok(2) failing on the layout)
    ("cminor", 2, "layout", 8), ("cminor", 1, "layout", 8),
    ("planes", 4, "-", 8), ("planes", 4, "-", 4),
    ("generic", 1, "-", 8),
]
DECODE_REQUIRED_LAYOUTS = [("planes", "nchw_window"), ("generic", "nchw_window_odd"), ("generic", "every_other_pixel_nchw"), ("cminor", "nhwc_off1"),
                           ("cminor", "nhwc_off2"), ("cminor", "nhwc_ld3"), ("c8", "nhwc_wide"), ("c8", "batch_every_other"), ("c8", "every_other_pixel_nhwc")]
DECODE_REQUIRED_TOPK = ["regs16", "lds32", "regs48", "lds16", "memory"]
EVEC4_REQUIRED = [(), ("channel stride",), ("E % 4",), ("strides % 4",), ("reid base",), ("emb base",)]      # the 16-byte path, and each clause failing ALONE


def test_the_strided_decodes_reached_every_stage1_kernel_width_and_key_storage():
    """Every form below ran — and passed — under a NON-packed heat layout in this session (the packed controls do not count).  A parametrisation that
    quietly ran nothing fails here."""
    reached = sorted(DECODE_REACHED)
    print("decode forms reached under a non-packed layout (stage 1, vec, cause, strip, top-k keys, heat layout):")
    for r in reached:
        print("   ", r)
    forms = {r[:4] for r in reached}
    missing = [f for f in DECODE_REQUIRED if f not in forms]
    missing += [f for f in DECODE_REQUIRED_LAYOUTS if f not in {(r[0], r[5]) for r in reached}]
    missing += [t for t in DECODE_REQUIRED_TOPK if t not in {r[4] for r in reached}]
    missing += [("e_vec4 fails only", c) for c in EVEC4_REQUIRED if c not in EVEC4_REACHED]
    print("e_vec4 clause sets failed:", sorted(EVEC4_REACHED))
    assert not missing, f"not reached under a non-packed layout: {missing}"
