"""GPU: cnl_draw_boxes_u8 and draw_detections (packed and YUV 4:2:0 frames) against tests/overlay_ref.py.

Every comparison is equality on BYTES: the corners are single fp32 operations and everything after them is integer, so there is no
tolerance to choose.  The paint kernel's tile is 64 x 16 samples: the (64, 96) frames have seams at x = 64 and y = 16, 32, 48, and
the YUV batches carry a (34, 132) frame beside the sizes of the packed ones so that the chroma planes (17 x 66) have seams too."""
import numpy as np
import pytest
import torch

import overlay_ref
import ref_cpu
import yuv_ref
import centernet_lightning_amd as cl

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (37, 53), (64, 96)]
YUV_SIZES = [(2, 2), (38, 54), (64, 96), (34, 132)]
NAN, INF = float("nan"), float("inf")
NUMBERS = (-1, 0, 9, 10, 1234567890)
PALETTE = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (3, 2, 1), (70, 240, 240)]
TEXT = (250, 251, 252)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def edge_boxes(H, W):
    """The hand-made set of one H x W frame."""
    return [
        (W * 0.25, H * 0.25, W * 0.6, H * 0.7),              # fully inside (its number is the ten-digit one: clipped by the right edge)
        (-5.0, H / 3.0, W / 3.0, H / 2.0), (W * 0.7, H / 4.0, W + 6.0, H / 2.0),          # crossing the left / right edge
        (W / 3.0, -4.0, W / 2.0, H / 3.0), (W / 4.0, H * 0.8, W / 2.0, H + 7.0),          # ... the top / bottom edge
        (-10.0, -10.0, W + 10.0, H + 10.0),                  # larger than the frame: nothing but (maybe) its tag is visible
        (-1.0, -1.0, float(W), float(H)),                    # ... by one pixel: the inner part of a thick ring is
        (W + 10.0, 1.0, W + 20.0, 5.0), (-30.0, -30.0, -5.0, -5.0), (1.0, H + 40.0, 5.0, H + 50.0),       # wholly outside
        (-1e30, -1e30, 1e30, 1e30), (1e30, 0.0, 2e30, 1.0),  # huge magnitudes
        (0.5, 1.5, 2.5, 3.5), (W / 2 + 0.5, H / 2 + 0.5, W / 2 + 4.5, H / 2 + 3.5), (W - 3.5, H - 2.5, W - 0.5, H - 0.5),     # x.5: half to even
        (1.0, 1.0, W - 2.0, H - 2.0), (3.0, 5.0, 3.0 + W / 3.0, 5.0 + H / 3.0),            # odd origins: the chroma rule
        (5.0, 1.0, 2.0, 4.0), (1.0, 5.0, 4.0, 2.0),          # inverted
        (3.4, 1.0, 2.6, 4.0),                                # inverted before rounding, one column after it: live
        (NAN, 0.0, 1.0, 1.0), (0.0, 0.0, 1.0, NAN), (0.0, -INF, 1.0, 1.0), (0.0, 0.0, INF, 1.0), (-INF, -INF, INF, INF),
        (60.0, 12.0, 70.0, 36.0), (120.0, 30.0, 131.0, 33.0),                                # across the tile seams, both directions
        (W * 0.2, H * 0.2, W * 0.7, H * 0.7), (W * 0.4, H * 0.4, W * 0.9, H * 0.9),          # two overlapping boxes
    ]


def make_slots(sizes, seed, n_random=20):
    """boxes [N, k, 4] float32, labels [N, k] int64 (negative ones too), numbers [N, k] int32, scores [N, k] float32, count [N] int32."""
    rng = np.random.default_rng(seed)
    boxes = []
    for (H, W) in sizes:
        cx, cy = rng.uniform(0, W, n_random), rng.uniform(0, H, n_random)
        bw, bh = rng.uniform(0, W, n_random) * rng.uniform(0, 1, n_random), rng.uniform(0, H, n_random) * rng.uniform(0, 1, n_random)
        rand = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=-1)
        boxes.append(np.concatenate([np.array(edge_boxes(H, W)), rand]).astype(np.float32))
    boxes = np.stack(boxes)
    N, k = boxes.shape[:2]
    labels = rng.integers(-20, 300, (N, k)).astype(np.int64)
    numbers = np.resize(np.array(NUMBERS, dtype=np.int32), (N, k)).copy()
    numbers[:, 0] = 1234567890
    scores = rng.uniform(0.2, 1, (N, k)).astype(np.float32)
    scores[:, 1] = np.float32(0.3)                                     # equal to the threshold: live
    scores[:, 2] = np.nextafter(np.float32(0.3), np.float32(0))        # one ulp below: dead
    scores[:, 3] = NAN                                                 # never live
    count = np.resize(np.array([k - 3, k - 10, k + 7, 5], dtype=np.int32), N)       # some, some, more than there are, few
    return boxes, labels, numbers, scores, count


def packed_frames(sizes, C, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, C), dtype=np.uint8) for (h, w) in sizes]


def assert_frames_equal(got, want, what=""):
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.shape == w.shape and g.dtype == np.uint8
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, n, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ----------------------------------------------------------------------------- packed frames
@pytest.mark.parametrize("thickness", [1, 2, 5])
def test_packed_frames_equal_the_reference(thickness):
    frames = packed_frames(SIZES, 3, seed=1)
    boxes, labels, numbers, scores, count = make_slots(SIZES, seed=2)
    tf = [dev(f) for f in frames]
    before = [f.clone() for f in tf]
    tb, tl, tn, ts, tc = dev(boxes), dev(labels), dev(numbers), dev(scores), dev(count)
    painted = 0
    for tag_scale in (0, 1, 3):
        for fill_alpha in (0, 64, 256):
            style = dict(thickness=thickness, fill_alpha=fill_alpha, tag_scale=tag_scale)
            got = cl.draw_detections(tf, tb, labels=tl, numbers=tn, scores=ts, score_threshold=0.3, count=tc, palette=PALETTE,
                                     text_color=TEXT, **style)
            want = overlay_ref.draw_reference(frames, boxes, PALETTE, TEXT, labels=labels, numbers=numbers, scores=scores, threshold=0.3,
                                              count=count, **style)
            assert isinstance(got, list)
            assert_frames_equal(got, want, style)
            painted += sum(int((w != f).any(-1).sum()) for w, f in zip(want, frames))
    assert painted > 0 and all(torch.equal(a, b) for a, b in zip(tf, before)), "inplace=False changed its input"
    # ungated, without labels (entry 0) and numbers, default palette and text colour
    got = cl.draw_detections(tf, tb, thickness=thickness)
    assert_frames_equal(got, overlay_ref.draw_reference(frames, boxes, cl.DEFAULT_PALETTE, thickness=thickness))


def test_the_cases_the_edge_set_is_there_for_occur():
    frames = packed_frames(SIZES, 3, seed=1)
    boxes, labels, numbers, scores, count = make_slots(SIZES, seed=2)
    H, W = SIZES[1]
    base = [np.zeros_like(f) for f in frames]
    # the ten-digit tag of slot 0 reaches the right edge of the 53-wide frame and is cut there
    one = overlay_ref.draw_reference(base[1:2], boxes[1:2, :1], [(9, 9, 9)], TEXT, numbers=numbers[1:2, :1], thickness=1, tag_scale=1)[0]
    assert int(round(W * 0.25)) + 61 > W and (one[:, W - 1] != 0).any()
    # gating: each gate kills slots that are otherwise drawn
    full = overlay_ref.draw_reference(base, boxes, [(9, 9, 9)], TEXT, tag_scale=0)
    by_count = overlay_ref.draw_reference(base, boxes, [(9, 9, 9)], TEXT, tag_scale=0, count=count)
    by_score = overlay_ref.draw_reference(base, boxes, [(9, 9, 9)], TEXT, tag_scale=0, scores=scores, threshold=0.3)
    assert any((a != b).any() for a, b in zip(full, by_count)) and any((a != b).any() for a, b in zip(full, by_score))
    # x.5 corners: (0.5, 1.5, 2.5, 3.5) -> (0, 2, 2, 4), not (1, 2, 3, 4)
    assert overlay_ref.corners(boxes[2, 12]) == (0, 2, 2, 4)
    live = [overlay_ref.corners(b) is not None for b in boxes[2]]
    assert 5 <= len(live) - sum(live) and sum(live) > 30


@pytest.mark.parametrize("C", [3, 4])
def test_a_batch_tensor_its_unaligned_slices_and_channel_3(C):
    """One [N, 37, 53, C] tensor: at C = 3 frame 1 starts at byte 5883, so its rows take the byte path; frame 2 the dword path."""
    sizes = [(37, 53)] * 3
    frames = packed_frames(sizes, C, seed=3)
    boxes, labels, numbers, _, _ = make_slots(sizes, seed=4)
    tb, tl, tn = dev(boxes), dev(labels), dev(numbers)
    style = dict(thickness=2, fill_alpha=64, tag_scale=1)
    want = overlay_ref.draw_reference(frames, boxes, PALETTE, TEXT, labels=labels, numbers=numbers, **style)
    batch = dev(np.stack(frames))
    keep = batch.clone()
    got = cl.draw_detections(batch, tb, labels=tl, numbers=tn, palette=PALETTE, text_color=TEXT, **style)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == tuple(batch.shape) and got.data_ptr() != batch.data_ptr()
    assert torch.equal(batch, keep)
    assert_frames_equal(list(got), want)
    # in place, as a list of slices of the tensor
    views = [batch[1], batch[2]]
    same = cl.draw_detections(views, tb[1:].contiguous(), labels=tl[1:].contiguous(), numbers=tn[1:].contiguous(), palette=PALETTE,
                              text_color=TEXT, inplace=True, **style)
    assert all(a is b for a, b in zip(same, views))
    assert torch.equal(batch[0], keep[0]), "a frame that was not given was painted"
    assert_frames_equal([batch[1], batch[2]], want[1:])
    # in place, the whole tensor
    same = cl.draw_detections(batch, tb, labels=tl, numbers=tn, palette=PALETTE, text_color=TEXT, inplace=True, **style)
    assert same is batch
    assert_frames_equal(list(batch), [want[0]] + overlay_ref.draw_reference(want[1:], boxes[1:], PALETTE, TEXT, labels=labels[1:],
                                                                            numbers=numbers[1:], **style))
    if C == 4:
        for n in range(3):
            assert np.array_equal(batch[n, :, :, 3].cpu().numpy(), frames[n][:, :, 3]), "channel 3 was modified"
        assert any((w[:, :, :3] != f[:, :, :3]).any() for w, f in zip(want, frames))


def test_rows_with_a_pitch_are_painted_in_place_and_the_padding_is_kept():
    frames = packed_frames(SIZES[1:], 3, seed=5)
    boxes, labels, numbers, _, _ = make_slots(SIZES[1:], seed=6)
    bufs = [torch.full((h, w + 7, 3), 0xEE, dtype=torch.uint8, device="cuda") for (h, w) in SIZES[1:]]
    views = [b[:, :f.shape[1]] for b, f in zip(bufs, frames)]
    for v, f in zip(views, frames):
        v.copy_(dev(f))
    cl.draw_detections(views, dev(boxes), labels=dev(labels), numbers=dev(numbers), palette=PALETTE, thickness=5, fill_alpha=64, inplace=True)
    want = overlay_ref.draw_reference(frames, boxes, PALETTE, labels=labels, numbers=numbers, thickness=5, fill_alpha=64)
    assert_frames_equal(views, want)
    assert all((b[:, f.shape[1]:] == 0xEE).all() for b, f in zip(bufs, frames)), "bytes beyond a row's pixels were written"


# ----------------------------------------------------------------------------- YUV frames
def pitched(a, extra):
    buf = torch.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], 0xEE, dtype=torch.uint8, device="cuda")
    buf[:, :a.shape[1]] = dev(a)
    return (buf, a.shape[1]), buf[:, :a.shape[1]]


def yuv_frames(planes, form):
    """-> (frames in the given form, [(the buffer behind a pitched plane, its visible width)])."""
    out, bufs = [], []
    for i, (y, u, v) in enumerate(planes):
        if form == "nv12":
            out.append(dev(yuv_ref.to_nv12(y, u, v)))
        elif form == "i420":
            out.append(dev(yuv_ref.to_i420(y, u, v)))
        elif form == "nv12_surface":                 # a decoder surface: pitch > width
            b, view = pitched(yuv_ref.to_nv12(y, u, v), 64 + 2 * i)
            out.append(view)
        elif form == "y_uv":                         # planes with their own pitches (the UV pitch odd: the byte path)
            (b, yv), (b2, uvv) = pitched(y, 37 + i), pitched(np.stack([u, v], axis=-1), 5 + i)
            out.append((yv, uvv))
            bufs.append(b2)
        else:                                        # "y_u_v"
            (b, yv), (b2, uv_), (b3, vv) = pitched(y, 13 + i), pitched(u, 9), pitched(v, 9)
            out.append((yv, uv_, vv))
            bufs += [b2, b3]
        if form not in ("nv12", "i420"):
            bufs.append(b)
    return out, bufs


def planes_of(frames, layout):
    return [tuple(p.cpu().numpy() for p in cl.split_planes(f, layout)) for f in frames]


def assert_planes_equal(got, want, what=""):
    for n, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip("yuv", g, w):
            bad = np.argwhere(a != b)
            assert a.shape == b.shape and len(bad) == 0, (what, n, name, len(bad), bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("form", ["nv12", "i420", "nv12_surface", "y_uv", "y_u_v"])
def test_yuv_frames_equal_the_reference(form):
    rng = np.random.default_rng(30 + len(form))
    planes = [yuv_ref.random_planes(rng, h, w) for (h, w) in YUV_SIZES]
    boxes, labels, numbers, scores, count = make_slots(YUV_SIZES, seed=7)
    layout = "i420" if form in ("i420", "y_u_v") else "nv12"
    tb, tl, tn, ts, tc = dev(boxes), dev(labels), dev(numbers), dev(scores), dev(count)
    frames, bufs = yuv_frames(planes, form)
    chroma_painted = 0
    for thickness, tag_scale, fill_alpha, matrix, full_range in ((1, 0, 0, "bt601", False), (2, 1, 64, "bt709", True), (5, 3, 256, "bt601", True),
                                                                 (2, 3, 0, "bt709", False)):
        style = dict(thickness=thickness, fill_alpha=fill_alpha, tag_scale=tag_scale)
        pal = [cl.rgb_to_yuv(c, matrix, full_range) for c in PALETTE]
        want = overlay_ref.draw_reference_yuv(planes, boxes, pal, cl.rgb_to_yuv(TEXT, matrix, full_range), labels=labels, numbers=numbers,
                                              scores=scores, threshold=0.3, count=count, **style)
        got = cl.draw_detections(frames, tb, labels=tl, numbers=tn, scores=ts, score_threshold=0.3, count=tc, palette=PALETTE, text_color=TEXT,
                                 pixel_format=layout, matrix=matrix, full_range=full_range, **style)
        assert isinstance(got, list) and len(got) == len(frames)
        for g, f in zip(got, frames):                # the form is kept
            assert type(g) is type(f) and (isinstance(f, torch.Tensor) and g.shape == f.shape or len(g) == len(f))
        assert_planes_equal(planes_of(got, layout), want, (form, style))
        assert_planes_equal(planes_of(frames, layout), planes, "inplace=False changed its input")
        chroma_painted += sum(int((w[1] != p[1]).sum()) for w, p in zip(want, planes))
    assert chroma_painted > 0
    # in place: the given memory is painted and returned; the pitch padding keeps its bytes
    same = cl.draw_detections(frames, tb, labels=tl, numbers=tn, palette=PALETTE, text_color=TEXT, pixel_format=layout, fill_alpha=64,
                              inplace=True)
    assert same is frames
    want = overlay_ref.draw_reference_yuv(planes, boxes, [cl.rgb_to_yuv(c) for c in PALETTE], cl.rgb_to_yuv(TEXT), labels=labels,
                                          numbers=numbers, fill_alpha=64)
    assert_planes_equal(planes_of(frames, layout), want, (form, "in place"))
    for buf, visible in bufs:
        assert (buf[:, visible:] == 0xEE).all(), "pitch padding was written"
    assert bufs or form in ("nv12", "i420")


# ----------------------------------------------------------------------------- order across scan chunks
def test_300_overlapping_boxes_keep_their_order_across_chunks():
    H, W = 64, 48
    rng = np.random.default_rng(8)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    k = 300
    x1, y1 = rng.uniform(-4, W / 2 - 2, k), rng.uniform(-4, H / 2 - 2, k)
    x2, y2 = rng.uniform(W / 2 + 2, W + 4, k), rng.uniform(H / 2 + 2, H + 4, k)       # every box holds the centre
    boxes = np.stack([x1, y1, x2, y2], axis=-1).astype(np.float32)[None]
    labels = rng.integers(0, 256, (1, k)).astype(np.int64)
    numbers = np.arange(k, dtype=np.int32)[None]
    palette = rng.integers(0, 256, (256, 3)).tolist()
    style = dict(thickness=2, fill_alpha=64, tag_scale=1)
    got = cl.draw_detections([dev(frame)], dev(boxes), labels=dev(labels), numbers=dev(numbers), palette=palette, text_color=TEXT, **style)
    want = overlay_ref.draw_reference([frame], boxes, palette, TEXT, labels=labels, numbers=numbers, **style)
    assert_frames_equal(got, want)
    # the order matters here: the slots applied first to last instead give another picture
    other = overlay_ref.draw_reference([frame], boxes[:, ::-1], palette, TEXT, labels=labels[:, ::-1], numbers=numbers[:, ::-1], **style)
    assert (other[0] != want[0]).any()
    # and the YUV planes of the same size, k beyond one chunk in every plane
    planes = [yuv_ref.random_planes(rng, H, W)]
    pal = [cl.rgb_to_yuv(c) for c in palette]
    got = cl.draw_detections([dev(yuv_ref.to_nv12(*planes[0]))], dev(boxes), labels=dev(labels), numbers=dev(numbers), palette=palette,
                             text_color=TEXT, pixel_format="nv12", **style)
    want = overlay_ref.draw_reference_yuv(planes, boxes, pal, cl.rgb_to_yuv(TEXT), labels=labels, numbers=numbers, **style)
    assert_planes_equal(planes_of(got, "nv12"), want)


# ----------------------------------------------------------------------------- degenerate and behavioural cases
def test_no_slots_and_no_frames_are_no_ops():
    frames = packed_frames(SIZES, 3, seed=9)
    tf = [dev(f) for f in frames]
    got = cl.draw_detections(tf, torch.zeros((3, 0, 4), device="cuda"))
    assert_frames_equal(got, frames)
    assert all(g.data_ptr() != f.data_ptr() for g, f in zip(got, tf))
    same = cl.draw_detections(tf, torch.zeros((3, 0, 4), device="cuda"), inplace=True)
    assert all(a is b for a, b in zip(same, tf))
    assert_frames_equal(tf, frames)
    assert cl.draw_detections([], torch.zeros((0, 5, 4), device="cuda")) == []
    empty = torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device="cuda")
    assert tuple(cl.draw_detections(empty, torch.zeros((0, 5, 4), device="cuda")).shape) == (0, 8, 8, 3)
    assert cl.draw_detections(empty, torch.zeros((0, 5, 4), device="cuda"), inplace=True) is empty
    # live boxes, all gated away: nothing is painted
    boxes = dev(np.tile(np.float32([0, 0, 2, 2]), (3, 9, 1)))
    got = cl.draw_detections(tf, boxes, count=torch.zeros((3,), dtype=torch.int32, device="cuda"), numbers=torch.ones((3, 9), dtype=torch.int32, device="cuda"))
    assert_frames_equal(got, frames)


def test_two_runs_give_identical_bytes():
    frames = packed_frames(SIZES, 3, seed=10)
    boxes, labels, numbers, scores, count = make_slots(SIZES, seed=11)
    tf, args = [dev(f) for f in frames], dict(labels=dev(labels), numbers=dev(numbers), fill_alpha=64, thickness=5, tag_scale=3)
    a = cl.draw_detections(tf, dev(boxes), **args)
    b = cl.draw_detections(tf, dev(boxes), **args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- end to end: detector -> overlay
def test_detections_are_drawn_end_to_end():
    torch.manual_seed(0)
    model = cl.build_centernet({"model": {"backbone": {"name": "resnet18"}, "neck": {"name": "simple"},
                                          "output_heads": {"heatmap": {"num_classes": 4}, "box_2d": {}}}})
    model.load_state_dict(ref_cpu.synth_state_dict(model.state_dict(), seed=0, calib_shape=(2, 3, 64, 64)))
    model = model.cuda()
    rng = np.random.default_rng(12)
    sizes = [(60, 90), (48, 40)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in sizes]
    tf = [dev(f) for f in frames]
    dets = model.detect_frames(tf, 64, 64, num_detections=20)
    boxes, labels, scores = dets["bboxes"].cpu().numpy(), dets["labels"].cpu().numpy(), dets["scores"].cpu().numpy()
    threshold = float(np.median(scores))
    got = model.draw_detections(tf, dets["bboxes"], labels=dets["labels"], scores=dets["scores"], score_threshold=threshold,
                                numbers=dets["labels"].to(torch.int32), fill_alpha=32)
    want = overlay_ref.draw_reference(frames, boxes, cl.DEFAULT_PALETTE, labels=labels, numbers=labels.astype(np.int32), scores=scores,
                                      threshold=threshold, fill_alpha=32)
    assert_frames_equal(got, want)
    live = scores >= np.float32(threshold)
    print(f"detect_frames -> overlay: threshold {threshold:.6g}, {int(live.sum())} live, {int((~live).sum())} dead slots, "
          f"{sum(int((w != f).any(-1).sum()) for w, f in zip(want, frames))} pixels painted")
    assert live.any() and (~live).any() and any((w != f).any() for w, f in zip(want, frames))
    # the same detections on the frames as NV12 surfaces, in place
    planes = [yuv_ref.random_planes(rng, h, w) for (h, w) in sizes]
    surfaces, _ = yuv_frames(planes, "nv12_surface")
    out = model.draw_detections(surfaces, dets["bboxes"], labels=dets["labels"], scores=dets["scores"], score_threshold=threshold,
                                pixel_format="nv12", inplace=True)
    assert out is surfaces
    want = overlay_ref.draw_reference_yuv(planes, boxes, [cl.rgb_to_yuv(c) for c in cl.DEFAULT_PALETTE], cl.rgb_to_yuv((255, 255, 255)),
                                          labels=labels, scores=scores, threshold=threshold)
    assert_planes_equal(planes_of(surfaces, "nv12"), want)
