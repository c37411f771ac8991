"""GPU: cnl_crop_boxes_u8 and crop_detections (packed and YUV 4:2:0 frames).

Every comparison is equality on BYTES (crops) and on integers (windows): the window rule is single fp32 operations, the target rule
float64, the pixels the integer resize — tests/crop_ref.py restates all three, so there is no tolerance to choose.  The YUV frames use
(38, 54) where the packed ones use (37, 53): 4:2:0 frames have even sizes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import crop_ref
import ref_cpu
import yuv_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _gather, _lib

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")

SIZES = [(2, 2), (16, 8), (37, 53), (120, 200), (270, 480)]
YUV_SIZES = [(2, 2), (16, 8), (38, 54), (120, 200), (270, 480)]
CROPS = [(128, 64), (64, 128), (32, 32), (20, 12), (1, 4)]
FILL = (114, 7, 201, 33)
NAN, INF = float("nan"), float("inf")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def edge_boxes(H, W):
    """The hand-made set of one H x W frame: live windows first, then the dead cases."""
    live = [
        (0.2, 0.2, 0.8, 0.8),                                # 1 x 1 at the origin: the byte-load path (w * C < 8), up-scaled > 8x
        (W - 0.9, H - 0.9, W - 0.1, H - 0.1),                # 1 x 1 at the last pixel
        (0.5, 0.5, 1.5, 1.5),                                # 2 x 2
        (W - 2.0, H - 2.0, W + 3.0, H + 3.0),                # 2 x 2 touching the right / bottom edge, clipped
        (W - 5.5, H - 3.5, float(W), float(H)),              # touching the right / bottom edge: the pulled-back 8-byte load
        (W / 2.0, 0.0, float(W), float(H)),                  # the right half
        (1.0, 1.0, W - 0.5, H - 0.5),                        # odd x0, y0
        (3.0, 5.0, 3.5 + W / 3.0, 5.5 + H / 3.0),            # odd x0, y0 again (dead on the frames smaller than that)
        (0.0, 0.0, float(W), float(H)),                      # the whole frame: down-scaled > 4x on the large frames
        (-10.0, -10.0, W + 10.0, H + 10.0),                  # ... from a box larger than the frame
        (-1e30, -1e30, 1e30, 1e30),                          # ... from huge magnitudes
        (0.5, 0.25, 0.5, 0.75),                              # x1 == x2 off an integer: one column
        (0.0, 0.0, 3.0, 3.0),                                # 3 x 3 (where the frame has it)
    ]
    dead = [
        (W + 10.0, 1.0, W + 20.0, 2.0), (-30.0, -30.0, -5.0, -5.0), (1e30, 0.0, 2e30, 1.0),            # wholly outside
        (1.5, 0.0, 0.5, 1.0), (0.0, 1.5, 1.0, 0.5),                                                    # inverted
        (1.0, 0.0, 1.0, 1.0), (0.0, 1.0, 1.0, 1.0),                                                    # x1 == x2 / y1 == y2 on an integer
        (NAN, 0.0, 1.0, 1.0), (0.0, 0.0, 1.0, NAN), (0.0, -INF, 1.0, 1.0), (0.0, 0.0, INF, 1.0), (-INF, -INF, INF, INF),
    ]
    return live, dead


def make_boxes(sizes, seed, n_random=20):
    """[N, k, 4] float32: per frame the edge set, then n_random seeded boxes (centres in the frame, sizes up to the frame's, so some
    reach over its edges), and how many of the edge set are dead."""
    rng = np.random.default_rng(seed)
    out = []
    for (H, W) in sizes:
        live, dead = edge_boxes(H, W)
        cx, cy = rng.uniform(0, W, n_random), rng.uniform(0, H, n_random)
        bw, bh = rng.uniform(0, W, n_random) * rng.uniform(0, 1, n_random), rng.uniform(0, H, n_random) * rng.uniform(0, 1, n_random)
        rand = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=-1)
        out.append(np.concatenate([np.array(live), np.array(dead), rand]).astype(np.float32))
    return np.stack(out), len(edge_boxes(4, 4)[1])


def packed_frames(sizes, C, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, C), dtype=np.uint8) for (h, w) in sizes]


def check(got, ref, boxes=None):
    crops, windows = got
    assert crops.dtype == torch.uint8 and windows.dtype == torch.int32 and crops.is_cuda and windows.is_cuda
    assert tuple(crops.shape) == ref[0].shape and tuple(windows.shape) == ref[1].shape
    w, c = windows.cpu().numpy(), crops.cpu().numpy()
    bad = np.argwhere((w != ref[1]).any(-1))
    assert len(bad) == 0, (bad[:5].tolist(), None if boxes is None else boxes[tuple(bad[0])].tolist(), w[tuple(bad[0])], ref[1][tuple(bad[0])])
    bad = np.argwhere(c != ref[0])
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


def assert_dead_slots_are_fill(crops, windows, fill, expect_dead):
    w, c = windows.cpu().numpy(), crops.cpu().numpy()
    dead = (w[..., 2] == 0)
    assert (w[dead] == 0).all() and (w[~dead, 2:] >= 1).all() and dead.sum() >= expect_dead and (~dead).any()
    assert (c[dead] == np.asarray(fill[:c.shape[-1]], dtype=np.uint8)).all()


# ----------------------------------------------------------------------------- packed frames against the reference
@pytest.mark.parametrize("size", CROPS)
def test_packed_crops_and_windows_equal_the_reference(size):
    frames = packed_frames(SIZES, 3, seed=1)
    boxes, n_dead = make_boxes(SIZES, seed=2)
    tf, tb = [dev(f) for f in frames], dev(boxes)
    for keep_aspect in (False, True):
        for pad in (0.0, 0.15):
            got = cl.crop_detections(tf, tb, size=size, pad=pad, keep_aspect=keep_aspect, fill=FILL[:3])
            ref = crop_ref.crop_reference(frames, boxes, size, pad=pad, keep_aspect=keep_aspect, fill=FILL)
            check(got, ref, boxes)
            assert_dead_slots_are_fill(*got, FILL, n_dead * len(SIZES))
    # the shapes the edge set is there for occur (windows are the same for every crop size; the last ref is pad 0.15, so look at pad 0)
    win = crop_ref.crop_reference(frames, boxes, (1, 4), fill=FILL)[1]
    for n, (H, W) in enumerate(SIZES):
        w = win[n][win[n][:, 2] > 0]
        assert ((w[:, 2] == 1) & (w[:, 3] == 1)).any() and (w == (0, 0, W, H)).all(-1).any()
        assert ((w[:, 0] + w[:, 2] == W) & (w[:, 1] + w[:, 3] == H) & (w[:, 0] > 0)).any()              # touches the right / bottom edge
        assert (w[:, 2] * 3 < 8).any() and (H < 2 or ((w[:, 2] == 2) & (w[:, 3] == 2)).any())           # narrow rows: byte loads
    w = win[-1][win[-1][:, 2] > 0]
    assert (w[:, 2] > 4 * size[1]).any() or (w[:, 3] > 4 * size[0]).any()                              # down-scaled by more than 4x
    assert size == (1, 4) or (w[:, 2] * 8 < size[1]).any() or (w[:, 3] * 8 < size[0]).any()            # up-scaled by more than 8x


@pytest.mark.parametrize("C", [1, 4])
def test_other_channel_counts_and_a_batch_tensor(C):
    frames = packed_frames(SIZES, C, seed=3 + C)
    boxes, n_dead = make_boxes(SIZES, seed=4)
    tf, tb = [dev(f) for f in frames], dev(boxes)
    for size, keep_aspect, pad in (((128, 64), False, 0.0), ((20, 12), True, 0.15), ((1, 4), False, 0.15)):
        got = cl.crop_detections(tf, tb, size=size, pad=pad, keep_aspect=keep_aspect, fill=FILL)
        check(got, crop_ref.crop_reference(frames, boxes, size, pad=pad, keep_aspect=keep_aspect, fill=FILL), boxes)
        assert_dead_slots_are_fill(*got, FILL, n_dead * len(SIZES))
    # one [N, h, w, C] tensor is N frames; black fill is the default (three values: a fourth channel has to be named)
    same = packed_frames([(37, 53)] * 3, C, seed=5)
    b3 = np.ascontiguousarray(np.repeat(boxes[2:3], 3, axis=0))
    got = cl.crop_detections(dev(np.stack(same)), dev(b3), size=(32, 32), **({"fill": 0} if C == 4 else {}))
    check(got, crop_ref.crop_reference(same, b3, (32, 32), fill=(0, 0, 0, 0)), b3)


# ----------------------------------------------------------------------------- YUV frames
def pitched(a, extra):
    buf = torch.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], 0xEE, dtype=torch.uint8, device="cuda")
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def yuv_frames(planes, form):
    out = []
    for i, (y, u, v) in enumerate(planes):
        if form == "nv12":
            out.append(dev(yuv_ref.to_nv12(y, u, v)))
        elif form == "i420":
            out.append(dev(yuv_ref.to_i420(y, u, v)))
        elif form == "nv12_surface":                 # a decoder surface: pitch > width
            out.append(pitched(yuv_ref.to_nv12(y, u, v), 64 + 2 * i))
        elif form == "y_uv":                         # planes with their own pitches
            out.append((pitched(y, 37 + i), pitched(np.stack([u, v], axis=-1), 5 + i)))
        else:                                        # "y_u_v"
            out.append((pitched(y, 13 + i), pitched(u, 9), pitched(v, 9)))
    return out


@pytest.mark.parametrize("form", ["nv12", "i420", "nv12_surface", "y_uv", "y_u_v"])
def test_yuv_crops_equal_the_reference_and_the_packed_entry_on_converted_frames(form):
    rng = np.random.default_rng(30 + len(form))
    planes = [yuv_ref.random_planes(rng, h, w) for (h, w) in YUV_SIZES]
    boxes, n_dead = make_boxes(YUV_SIZES, seed=6)
    frames, tb = yuv_frames(planes, form), dev(boxes)
    layout = "i420" if form in ("i420", "y_u_v") else "nv12"
    odd = 0
    for size, keep_aspect, pad, matrix, full_range in (((128, 64), False, 0.0, "bt601", False), ((20, 12), True, 0.15, "bt709", True),
                                                       ((32, 32), True, 0.0, "bt601", True)):
        got = cl.crop_detections(frames, tb, size=size, pad=pad, keep_aspect=keep_aspect, fill=FILL[:3], pixel_format=layout, matrix=matrix,
                                 full_range=full_range)
        ref = crop_ref.crop_reference_yuv(planes, boxes, size, matrix, full_range, pad=pad, keep_aspect=keep_aspect, fill=FILL)
        check(got, ref, boxes)
        assert_dead_slots_are_fill(*got, FILL, n_dead * len(YUV_SIZES))
        rgb = [dev(yuv_ref.yuv420_to_rgb(y, u, v, matrix, full_range)) for (y, u, v) in planes]
        want = cl.crop_detections(rgb, tb, size=size, pad=pad, keep_aspect=keep_aspect, fill=FILL[:3])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        live = ref[1][..., 2] > 0
        odd += int(((ref[1][live][:, 0] % 2 == 1) | (ref[1][live][:, 1] % 2 == 1)).sum())
    assert odd > 0, "no window with an odd origin was exercised"


# ----------------------------------------------------------------------------- against letterbox_uint8 of the sliced frames
@pytest.mark.parametrize("size", [(128, 64), (64, 128), (32, 32)])
def test_keep_aspect_crops_equal_letterbox_uint8_of_the_slices(size):
    frames = packed_frames(SIZES, 3, seed=7)
    boxes, _ = make_boxes(SIZES, seed=8)
    tf = [dev(f) for f in frames]
    crops, windows = cl.crop_detections(tf, dev(boxes), size=size, pad=0.15, keep_aspect=True, fill=FILL[:3])
    w = windows.cpu().numpy()
    slots = [(n, j) for n in range(w.shape[0]) for j in range(w.shape[1]) if w[n, j, 2] > 0]
    slices = [tf[n][w[n, j, 1]:w[n, j, 1] + w[n, j, 3], w[n, j, 0]:w[n, j, 0] + w[n, j, 2]] for (n, j) in slots]
    canvas, _ = cl.letterbox.letterbox_uint8(slices, size[0], size[1], fill=FILL[:3])
    idx = torch.tensor(slots, device="cuda")
    assert len(slots) > 100 and torch.equal(crops[idx[:, 0], idx[:, 1]], canvas)


# ----------------------------------------------------------------------------- gating
def test_gating_by_count_by_scores_and_by_both():
    frames = packed_frames(SIZES, 3, seed=9)
    boxes, _ = make_boxes(SIZES, seed=10)
    N, k = boxes.shape[:2]
    rng = np.random.default_rng(11)
    scores = rng.uniform(0, 1, (N, k)).astype(np.float32)
    scores[:, 0] = np.float32(0.3)                                     # equal to the threshold: live
    scores[:, 1] = np.nextafter(np.float32(0.3), np.float32(0))        # one ulp below: dead
    scores[:, 2] = NAN                                                 # never live
    count = np.array([0, 5, k, k + 7, 13], dtype=np.int32)            # none, some, all, more than there are, some
    tf, tb, ts, tc = [dev(f) for f in frames], dev(boxes), dev(scores), dev(count)
    plain = crop_ref.crop_reference(frames, boxes, (20, 12), fill=FILL)
    seen = []
    for kw, rkw in (({"count": tc}, {"count": count}), ({"scores": ts, "score_threshold": 0.3}, {"scores": scores, "threshold": 0.3}),
                    ({"count": tc, "scores": ts, "score_threshold": 0.3}, {"count": count, "scores": scores, "threshold": 0.3})):
        got = cl.crop_detections(tf, tb, size=(20, 12), fill=FILL[:3], **kw)
        ref = crop_ref.crop_reference(frames, boxes, (20, 12), fill=FILL, **rkw)
        check(got, ref, boxes)
        seen.append(int((ref[1][..., 2] > 0).sum()))
    w = got[1].cpu().numpy()
    assert w[:, 0, 2].max() > 0 and (w[:, 1] == 0).all() and (w[:, 2] == 0).all() and (w[0] == 0).all()
    assert seen[2] < seen[0] < int((plain[1][..., 2] > 0).sum()) and seen[2] < seen[1]     # each input gates, together they gate more


# ----------------------------------------------------------------------------- the C ABI: every byte written, nothing beyond
@pytest.mark.parametrize("yuv", [False, True])
def test_c_abi_writes_every_crop_byte_and_no_guard_byte(yuv):
    sizes = YUV_SIZES
    boxes, _ = make_boxes(sizes, seed=12)
    N, k = boxes.shape[:2]
    rng = np.random.default_rng(13)
    keep = []
    if yuv:         # grey frames: Y 16..99 without chroma converts to bytes <= 97, so no source byte is 0xEE
        planes = [(rng.integers(16, 100, (h, w), dtype=np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8))
                  for (h, w) in sizes]
        rec = np.zeros((N, 9), dtype=np.int64)
        pl = []
        for (y, u, v) in planes:
            ty, tuv = dev(y), dev(np.stack([u, v], axis=-1))
            keep += [ty, tuv]
            pl.append((ty.data_ptr(), tuv.data_ptr(), tuv.data_ptr() + 1, y.shape[1], y.shape[1], 2))
        _gather.pack_yuv(rec, [(n, 0, 0, h, w, 1, 1, 0, 0) for n, (h, w) in enumerate(sizes)], pl)
        frames = [yuv_ref.yuv420_to_rgb(*p) for p in planes]
        coef = (ctypes.c_int32 * 6)(*cl.yuv_coefficients())
    else:
        frames = [rng.integers(0, 200, (h, w, 3), dtype=np.uint8) for (h, w) in sizes]
        rec = np.zeros((N, 5), dtype=np.int64)
        keep = [dev(f) for f in frames]
        _gather.pack_plain(rec, [(n, 0, 0, h, w, 1, 1, 0, 0) for n, (h, w) in enumerate(sizes)], [(t.data_ptr(), t.shape[1] * 3) for t in keep])
        coef = None
    lib = _lib.load()
    table, tb = dev(rec), dev(boxes)
    for (ch, cw), keep_aspect in (((128, 64), 0), ((20, 12), 1), ((1, 4), 0)):
        guard, body = 4096, N * k * ch * cw * 3
        buf = torch.full((guard + body + guard,), 0xEE, dtype=torch.uint8, device="cuda")
        windows = torch.full((N * k * 4 + 64,), -7, dtype=torch.int32, device="cuda")
        records = torch.empty((N * k * rec.shape[1] + 8,), dtype=torch.int64, device="cuda")
        _lib.check(lib.cnl_crop_boxes_u8(table.data_ptr(), tb.data_ptr(), None, 0.0, None, N, k, 3, coef, 0.15, keep_aspect, records.data_ptr(),
                                         windows.data_ptr(), buf.data_ptr() + guard, ch, cw, 0x030201,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "cnl_crop_boxes_u8")
        torch.cuda.synchronize()
        assert (buf[:guard] == 0xEE).all() and (buf[-guard:] == 0xEE).all(), "bytes outside the crops were written"
        assert not (buf[guard:-guard] == 0xEE).any(), "a crop byte was not written"
        assert (windows[N * k * 4:] == -7).all()
        ref = crop_ref.crop_reference(frames, boxes, (ch, cw), pad=0.15, keep_aspect=bool(keep_aspect), fill=(1, 2, 3))
        assert np.array_equal(buf[guard:-guard].view(N, k, ch, cw, 3).cpu().numpy(), ref[0])
        assert np.array_equal(windows[:N * k * 4].view(N, k, 4).cpu().numpy(), ref[1])


# ----------------------------------------------------------------------------- more slots than one launch takes; none at all
def test_66000_slots_are_launched_in_chunks():
    frame = packed_frames([(37, 53)], 3, seed=14)
    distinct, _ = make_boxes([(37, 53)], seed=15)                      # 45 boxes, repeated: the reference works each out once
    k = 66000
    boxes = np.ascontiguousarray(np.resize(distinct[0], (k, 4))[None])
    boxes[0, -1] = (0.0, 0.0, 53.0, 37.0)                              # the last slot of the last chunk is live
    got = cl.crop_detections([dev(frame[0])], dev(boxes), size=(1, 4), fill=FILL[:3])
    ref = crop_ref.crop_reference(frame, boxes, (1, 4), fill=FILL)
    check(got, ref)
    assert ref[1][0, 65535:, 2].max() > 0 and ref[1][0, -1, 2] == 53


def test_no_slots_and_an_all_dead_batch():
    frames = packed_frames(SIZES[:3], 3, seed=16)
    tf = [dev(f) for f in frames]
    crops, windows = cl.crop_detections(tf, torch.zeros((3, 0, 4), device="cuda"), size=(20, 12))
    torch.cuda.synchronize()
    assert tuple(crops.shape) == (3, 0, 20, 12, 3) and tuple(windows.shape) == (3, 0, 4)
    boxes = np.zeros((3, 9, 4), dtype=np.float32)                      # zero boxes, as detect_tiled leaves past a frame's count
    boxes[:, 3] = NAN
    boxes[:, 4] = (60.0, 60.0, 70.0, 70.0)
    got = cl.crop_detections(tf, dev(boxes), size=(20, 12), fill=FILL[:3], keep_aspect=True, pad=0.15)
    check(got, crop_ref.crop_reference(frames, boxes, (20, 12), fill=FILL, keep_aspect=True, pad=0.15))
    assert (got[1] == 0).all() and (got[0] == torch.tensor(FILL[:3], dtype=torch.uint8, device="cuda")).all()
    live = dev(np.tile(np.float32([0, 0, 2, 2]), (3, 9, 1)))           # live boxes, all gated away
    got = cl.crop_detections(tf, live, size=(20, 12), count=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    assert (got[1] == 0).all() and (got[0] == 0).all()


# ----------------------------------------------------------------------------- end to end: detector -> crops
def test_detections_of_nv12_frames_are_cropped_end_to_end():
    torch.manual_seed(0)
    model = cl.build_centernet(os.path.join(CONFIGS, "tracking_resnet34_fpn.yaml"))
    model.load_state_dict(ref_cpu.synth_state_dict(model.state_dict(), seed=0, calib_shape=(2, 3, 128, 128)))
    model = model.cuda()
    sizes = [(270, 480), (120, 200), (300, 400)]
    rng = np.random.default_rng(17)
    planes = [yuv_ref.random_planes(rng, h, w) for (h, w) in sizes]
    frames = yuv_frames(planes, "nv12_surface")
    dets = model.detect_frames(frames, 256, 320, num_detections=40, pixel_format="nv12")
    boxes, scores = dets["bboxes"].cpu().numpy(), dets["scores"].cpu().numpy()
    threshold = float(np.median(scores))
    got = model.crop_detections(frames, dets["bboxes"], scores=dets["scores"], score_threshold=threshold, pad=0.15, pixel_format="nv12")
    ref = crop_ref.crop_reference_yuv(planes, boxes, (128, 64), scores=scores, threshold=threshold, pad=0.15)
    check(got, ref, boxes)
    live = ref[1][..., 2] > 0
    print(f"detect_frames -> crops: threshold {threshold:.6g}, {int(live.sum())} live, {int((~live).sum())} dead slots")
    assert live.any() and (~live).any()
    # sliced inference: rows past a frame's count are dead
    tiled = model.detect_tiled(frames, tile=(128, 128), batch=16, max_detections=300, score_threshold=threshold, pixel_format="nv12")
    boxes, count = tiled["bboxes"].cpu().numpy(), tiled["count"].cpu().numpy()
    got = model.crop_detections(frames, tiled["bboxes"], count=tiled["count"], keep_aspect=True, fill=FILL[:3], pixel_format="nv12")
    ref = crop_ref.crop_reference_yuv(planes, boxes, (128, 64), count=count, keep_aspect=True, fill=FILL)
    check(got, ref, boxes)
    live = ref[1][..., 2] > 0
    print(f"detect_tiled -> crops: counts {count.tolist()}, {int(live.sum())} live, {int((~live).sum())} dead slots")
    assert live.any() and (~live).any()
