"""Whole training steps on the device against the float64 twin of tests/train_step_ref.py, step by step: TrainAugment / TrainWarp, a small torch
model in fp32, DetectionLoss / TrackingLoss and torch.optim.SGD(momentum 0.9), T = 8 steps of N = 4 canvases of 64 x 160 (a 16 x 40 map: two tile
rows, two tile columns, the second one partial) cut from six frames of other sizes, with 0 to 12 source boxes per frame, a Gmax that changes from
step to step and, in the detection loop, one step without a box in any image.

In lock step the device's canvas, targets, loss values and map gradients are held against the restatements on the device model's OWN maps, within the
bounds of tests/test_gpu_loss.py, test_gpu_loss_grad.py and test_gpu_reid_loss.py (imported, not copied).  Over the trajectory the bound is
train_step_ref.bound: 4 x max(the fp32 host loop's own distance from the twin, T x 2^-23), computed in the run itself; what that bound still catches
is shown without a device by tests/test_train_step_host.py.

Measured on an MI355X (d: max over parameter tensors of max |theta - theta64| / max |theta64| after the 8 steps; gaps: per-step |total - total64| /
|total64|; d32 and the host gaps are those of the fp32 host loop in the same run, and the bound is 4 x max(d32, 8 x 2^-23) = 3.8e-6 in every line):
    detection   d32 3.2e-07   d_gpu 4.2e-07   loss gaps, host up to 4.2e-08, device 5.7e-10 2.5e-09 8.5e-10 3.2e-09 1.5e-11 1.2e-08 6.1e-09 6.1e-08
    tracking    d32 2.3e-07   d_gpu 2.0e-07   loss gaps, host up to 6.7e-08, device 3.0e-10 4.3e-09 8.9e-09 5.2e-09 5.7e-09 9.8e-09 2.6e-09 4.1e-08
    tracking, running statistics:  host 2.3e-07, device 1.6e-07
In lock step every map gradient, classifier gradient and running statistic of the 16 steps was fl32 of the restatement (no element off).
"""
import numpy as np
import pytest
import torch

import loss_grad_ref
import loss_ref
import reid_loss_ref
import test_gpu_loss as value_bounds
import test_gpu_loss_grad as grad_bounds
import test_gpu_reid_loss as reid_bounds
import train_step_ref as R
import centernet_lightning_amd as cl

pytestmark = pytest.mark.gpu
PLAN_FIELDS = {"augment": ("n_place", "frame", "window", "dest", "flip", "colour", "holes"), "warp": ("n_place", "frame", "window", "dest", "fwd", "inv", "colour", "holes")}
CLASSIFIER = {"W1": (0, "weight"), "gamma": (1, "weight"), "beta": (1, "bias"), "running_mean": (1, "running_mean"), "running_var": (1, "running_var"),
              "W2": (3, "weight"), "b2": (3, "bias")}


# ----------------------------------------------------------------------------- helpers
def device_frames(indices):
    return [torch.from_numpy(R.frames()[f]).cuda() for f in indices]


def num(t):
    return float(t.detach())


def bits(t):
    return t.detach().contiguous().cpu().numpy()


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tensor_of(reid_module, key):
    index, name = CLASSIFIER[key]
    return getattr(reid_module.classifier[index], name)


def reid_criterion():
    """ReIDLoss(8, 20, loss_weight=0.7) in .train(), holding the twin's initial classifier."""
    module = cl.ReIDLoss(R.D, R.K, loss_weight=R.REID_WEIGHT, stride=R.STRIDE).cuda()
    with torch.no_grad():
        for k, v in R.classifier_values().items():
            tensor_of(module, k).copy_(torch.from_numpy(v))
    return module.train()


def classifier_numpy(module):
    return {k: tensor_of(module, k).detach().cpu().numpy().copy() for k in reid_loss_ref.KEYS}


def device_dict(batch, with_ids):
    keys = ("boxes", "labels", "count") + (("ids",) if with_ids else ())
    return {k: torch.from_numpy(batch[k]).cuda() for k in keys}


def check_batch(kind, plan, canvas, targets, batch):
    """The transform drew the twin's plan; canvas and targets are the restatement's, byte for byte, the zeros beyond count included."""
    for f in PLAN_FIELDS[kind]:
        assert np.array_equal(getattr(plan, f), getattr(batch["plan"], f)), f
    assert np.array_equal(canvas.cpu().numpy(), batch["canvas"])
    assert np.array_equal(targets["boxes"].cpu().numpy().view(np.uint64), batch["boxes"].view(np.uint64))
    assert np.array_equal(targets["labels"].cpu().numpy(), batch["labels"]) and np.array_equal(targets["count"].cpu().numpy(), batch["count"])
    assert targets["count"].dtype == torch.int32 and ("ids" in targets) == (batch["ids"] is not None)
    if batch["ids"] is not None:
        assert np.array_equal(targets["ids"].cpu().numpy(), batch["ids"])


def check_detection(maps, out, batch, what, total=True):
    """Values and map gradients against loss_ref / loss_grad_ref on the device model's own maps -> the restated value dict"""
    heat, box = bits(maps["heatmap"]), bits(maps["box_2d"])
    tg = R.list_targets(batch["boxes"], batch["labels"], batch["count"])
    want = loss_ref.detection_loss(heat, box, tg, **R.DETECTION)
    totals = [num(out["heatmap"]), num(out["box_2d"]), num(out["total"]) if total else want["total"]]
    value_bounds.check_result(out["per_image"].cpu().numpy(), totals, out["skipped"], want)
    want_grad = loss_grad_ref.detection_loss_grad(heat, box, tg, heatmap_scale=R.DETECTION.get("heatmap_loss_weight", 1.0),
                                                  box_scale=R.DETECTION["box_loss_weight"], **R.DETECTION)
    grad_bounds.check(bits(maps["heatmap"].grad), bits(maps["box_2d"].grad), out["skipped"], want_grad, R.DETECTION, what)
    return want


def check_reid(maps, out, batch, before, module, t, what):
    """The re-ID half of a step against reid_loss_ref on the device's own map and the classifier as it was before the step -> the restated value"""
    args = (bits(maps["reid"]), batch["boxes"], batch["ids"], batch["count"], before)
    kw = dict(training=True, stride=R.STRIDE, bn_eps=R.BN_EPS, momentum=R.BN_MOMENTUM)
    want, want_grad = reid_loss_ref.reid_loss(*args, **kw), reid_loss_ref.reid_loss_grad(*args, scale=R.REID_WEIGHT, **kw)
    np.testing.assert_allclose(num(out["reid"]), want["reid"], rtol=reid_bounds.VALUE_RTOL, err_msg=what)
    assert (int(out["num_rows"]), int(out["correct"]), int(out["reid_skipped"])) == (want["num_rows"], want["correct"], want["skipped"]), what
    g = bits(maps["reid"].grad)
    reid_bounds.within(g, want_grad["reid"], what + " d reid")
    unread = np.broadcast_to(~want_grad["read"][:, None], g.shape)
    assert (g[unread] == 0).all() and not np.signbit(g[unread]).any(), what
    for k in R.PARAMS:
        reid_bounds.within(bits(tensor_of(module, k).grad), want_grad[k], f"{what} d {k}")
    reid_bounds.within(bits(tensor_of(module, "running_mean")), want["running_mean64"], what + " running_mean")
    reid_bounds.within(bits(tensor_of(module, "running_var")), want["running_var64"], what + " running_var")
    assert want["stepped"] == 1 and int(module.classifier[1].num_batches_tracked) == t + 1, what
    return want


def check_trajectory(name, totals, got, kind, stats=None):
    """The per-step totals and the final parameters (and statistics) against the twin, within 4 x max(the fp32 host loop's distance, T 2^-23)."""
    twin, yard = R.reference_loops(kind)
    g32, d32 = max(R.loss_gaps(yard["losses"], twin["losses"])), R.distance(yard["params"], twin["params"])
    gaps = R.loss_gaps([{"total": v} for v in totals], twin["losses"])
    d_gpu = R.distance(got, twin["params"])
    print(f"{name}: twin totals {[round(float(v['total']), 4) for v in twin['losses']]}")
    print(f"{name}: loss gaps, fp32 host {g32:.3e}, device {max(gaps):.3e} (per step {[f'{g:.1e}' for g in gaps]}), bound {R.bound(g32):.3e}")
    print(f"{name}: parameters, d32 {d32:.3e}, d_gpu {d_gpu:.3e}, bound {R.bound(d32):.3e}")
    assert max(gaps) <= R.bound(g32), (gaps, R.bound(g32))
    assert d_gpu <= R.bound(d32), (d_gpu, R.bound(d32))
    if stats is not None:
        s32, s_gpu = R.distance(yard["stats"][-1], twin["stats"][-1]), R.distance(stats, twin["stats"][-1])
        print(f"{name}: running statistics, fp32 host {s32:.3e}, device {s_gpu:.3e}, bound {R.bound(s32):.3e}")
        assert s_gpu <= R.bound(s32), (s_gpu, R.bound(s32))


def model_tensors(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.named_parameters()}


# ----------------------------------------------------------------------------- a: detection, in lock step
def test_detection_steps_in_lock_step_with_the_twin():
    data = R.loop_batches("augment")
    assert any(int(b["count"].sum()) == 0 for b in data) and any(a["boxes"].shape[1] > b["boxes"].shape[1] for a, b in zip(data, data[1:]))
    augment = cl.TrainAugment(R.HEIGHT, R.WIDTH, seed=R.SEEDS["augment"], **R.AUGMENT)
    model = R.TinyNet(R.C).cuda()
    criterion = cl.DetectionLoss(**R.DETECTION)
    optimiser = torch.optim.SGD(model.parameters(), lr=R.LR, momentum=R.MOMENTUM)
    totals, skipped = [], 0
    for t, batch in enumerate(data):
        canvas, targets = augment(device_frames(batch["frames"]), R.step_targets(t, False, R.EMPTY_STEP))
        check_batch("augment", augment.last_plan, canvas, targets, batch)
        optimiser.zero_grad(set_to_none=True)
        maps, _ = model(canvas)
        assert not maps["heatmap"].is_contiguous() and not maps["box_2d"].is_contiguous()
        for m in maps.values():
            m.retain_grad()
        out = criterion(maps, targets)
        out["total"].backward()
        check_detection(maps, out, batch, f"step {t}")
        skipped += int(out["skipped"])
        optimiser.step()
        totals.append(num(out["total"]))
    assert skipped == 0
    check_trajectory("detection", totals, model_tensors(model), "augment")


# ----------------------------------------------------------------------------- b: tracking, in lock step
def test_tracking_steps_in_lock_step_with_the_twin():
    data = R.loop_batches("warp")
    assert any(a["boxes"].shape[1] > b["boxes"].shape[1] for a, b in zip(data, data[1:])) and any((b["ids"] == -1).any() for b in data)
    warp = cl.TrainWarp(R.HEIGHT, R.WIDTH, seed=R.SEEDS["warp"], **R.WARP)
    model = R.TinyNet(R.C, R.D).cuda()
    reid = reid_criterion()
    criterion = cl.TrackingLoss(R.DETECTION, reid).train()
    optimiser = torch.optim.SGD(list(model.parameters()) + list(reid.parameters()), lr=R.LR, momentum=R.MOMENTUM)
    totals, skipped, seen = [], 0, []
    for t, batch in enumerate(data):
        canvas, targets = warp(device_frames(batch["frames"]), R.step_targets(t, True))
        check_batch("warp", warp.last_plan, canvas, targets, batch)
        before = classifier_numpy(reid)
        optimiser.zero_grad(set_to_none=True)
        maps, _ = model(canvas)
        for m in maps.values():
            m.retain_grad()
        out = criterion(maps, targets)
        out["total"].backward()
        want = check_detection(maps, out, batch, f"step {t}", total=False)
        want_reid = check_reid(maps, out, batch, before, reid, t, f"step {t}")
        np.testing.assert_allclose(num(out["total"]), want["total"] + R.REID_WEIGHT * want_reid["reid"], rtol=value_bounds.RTOL)
        skipped += int(out["skipped"]) + int(out["reid_skipped"])
        optimiser.step()
        totals.append(num(out["total"]))
        seen.append((canvas, targets))
    assert skipped == 0
    got = model_tensors(model)
    got.update({"classifier." + k: tensor_of(reid, k).detach().cpu().numpy().astype(np.float64) for k in R.PARAMS})
    check_trajectory("tracking", totals, got, "warp", {k: tensor_of(reid, k).cpu().numpy().astype(np.float64) for k in R.STATS})

    # validation after the last step: no re-ID loss, and the epoch means of a meter
    criterion.eval()
    frozen = classifier_numpy(reid)
    detection, meter = cl.DetectionLoss(**R.DETECTION), cl.LossMeter(**R.DETECTION)
    sums = np.zeros(3)
    with torch.no_grad():
        for (canvas, targets), batch in zip(seen[-2:], data[-2:]):
            maps, _ = model(canvas)
            a, b = criterion(maps, targets, ignore_reid=True), detection(maps, targets)
            for k in ("heatmap", "box_2d", "total", "per_image", "skipped"):
                assert same_bits(a[k], b[k]), k
            assert float(a["reid"]) == 0.0
            meter.update(maps, targets)
            want = loss_ref.detection_loss(bits(maps["heatmap"]), bits(maps["box_2d"]), R.list_targets(batch["boxes"], batch["labels"], batch["count"]), **R.DETECTION)
            sums += R.N * np.array([want["heatmap"], want["box_2d"], want["total"]])
    metrics = meter.get_metrics()
    np.testing.assert_allclose([metrics[k] for k in cl.LossMeter.metric_names], sums / (2 * R.N), rtol=value_bounds.RTOL)
    after = classifier_numpy(reid)
    assert all(np.array_equal(frozen[k], after[k]) for k in frozen) and int(reid.classifier[1].num_batches_tracked) == R.T


# ----------------------------------------------------------------------------- c: orders a real loop uses
def fixed_maps(emb):
    """The head tensor of the model at step 0 on the first "warp" canvas, as a leaf, and how to slice it."""
    model = R.TinyNet(R.C, emb).cuda()
    with torch.no_grad():
        _, y = model(torch.from_numpy(R.loop_batches("warp")[0]["canvas"]).cuda())

    def leaf():
        v = y.clone().requires_grad_()
        maps = {"heatmap": v[:, :R.C], "box_2d": v[:, R.C:R.C + 4]}
        if emb:
            maps["reid"] = v[:, R.C + 4:]
        return v, maps

    return leaf


def within_one_ulp_of_the_sum(got, a, b, what):
    total = bits(a).astype(np.float64) + bits(b).astype(np.float64)
    err = np.abs(bits(got).astype(np.float64) - total)
    assert (err <= np.spacing(np.abs(total).astype(np.float32)).astype(np.float64)).all(), (what, float(err.max()))


def test_accumulated_gradients_are_the_sum_of_the_single_ones():
    data = R.loop_batches("warp")
    leaf = fixed_maps(R.D)
    reid = reid_criterion()
    criterion = cl.TrackingLoss(R.DETECTION, reid).train()
    A, B = device_dict(data[0], True), device_dict(data[1], True)
    alone = []
    for targets in (A, B):
        v, maps = leaf()
        reid.zero_grad(set_to_none=True)
        criterion(maps, targets)["total"].backward()
        alone.append([v.grad.clone()] + [tensor_of(reid, k).grad.clone() for k in R.PARAMS])
    assert not torch.equal(alone[0][0], alone[1][0])
    v, maps = leaf()
    reid.zero_grad(set_to_none=True)
    out_a = criterion(maps, A)
    out_b = criterion(maps, B)
    out_b["total"].backward()
    out_a["total"].backward()
    for got, a, b, what in zip([v.grad] + [tensor_of(reid, k).grad for k in R.PARAMS], alone[0], alone[1], ("maps",) + R.PARAMS):
        within_one_ulp_of_the_sum(got, a, b, what)


@pytest.mark.parametrize("kind", ["augment", "warp"])
def test_refilling_the_out_buffers_before_the_backward_keeps_the_forwards_targets(kind):
    """A loop that reuses augment_batch's / warp_batch's out= buffers overwrites step A's targets with step B's before A's backward runs: the criteria
    keep their own copy of padded device targets, so the gradient is the one of A's targets."""
    data = R.loop_batches(kind, empty=False)
    i, j = next((i, j) for i in range(R.T) for j in range(i + 1, R.T) if data[i]["boxes"].shape == data[j]["boxes"].shape)
    run = cl.augment_batch if kind == "augment" else cl.warp_batch
    with_ids = kind == "warp"
    leaf = fixed_maps(R.D if with_ids else 0)
    reid = reid_criterion() if with_ids else None
    criterion = cl.TrackingLoss(R.DETECTION, reid).train() if with_ids else cl.DetectionLoss(**R.DETECTION)

    def batch(k, out=None):
        return run(device_frames(data[k]["frames"]), data[k]["plan"], R.step_targets(k, with_ids), out=out)

    def grads(targets, refill):
        v, maps = leaf()
        if reid is not None:
            reid.zero_grad(set_to_none=True)
        out = criterion(maps, targets)
        if refill:
            batch(j, buffers)
        out["total"].backward()
        return [v.grad.clone()] + ([tensor_of(reid, k).grad.clone() for k in R.PARAMS] if reid is not None else [])

    canvas, targets = batch(i)
    buffers = dict(targets, canvas=canvas)
    clean_a = grads({k: v.clone() for k, v in targets.items()}, False)
    got = grads(targets, True)
    check_batch(kind, data[j]["plan"], buffers["canvas"], {k: buffers[k] for k in targets}, data[j])          # the buffers now hold step B
    clean_b = grads({k: v.clone() for k, v in targets.items()}, False)
    assert not torch.equal(clean_a[0], clean_b[0])
    for g, a in zip(got, clean_a):
        assert same_bits(g, a)


def test_loss_scaling_enters_before_the_one_rounding():
    data = R.loop_batches("warp")
    leaf = fixed_maps(0)
    criterion = cl.DetectionLoss(**R.DETECTION)
    targets = device_dict(data[0], False)

    def grad_of(value):
        v, maps = leaf()
        value(criterion(maps, targets)).backward()
        return v.grad, maps

    plain, _ = grad_of(lambda out: out["total"])
    assert float(plain.abs().min()) == 0.0 and float(plain[plain != 0].abs().min()) > 2.0 ** -100          # nowhere near the subnormals
    up, _ = grad_of(lambda out: out["total"] * 1024)
    down, _ = grad_of(lambda out: out["total"] / 8)
    assert same_bits(up, plain * 1024) and same_bits(down, plain / 8)
    mixed, maps = grad_of(lambda out: out["heatmap"] + 0.1 * out["box_2d"])
    direct = cl.detection_loss_grad(maps["heatmap"].detach(), maps["box_2d"].detach(), targets, heatmap_scale=1.0, box_scale=0.1, **R.DETECTION)
    assert same_bits(mixed[:, :R.C], direct["heatmap_grad"]) and same_bits(mixed[:, R.C:], direct["box_2d_grad"])


@pytest.mark.parametrize("kind", ["augment", "warp"])
def test_a_side_stream_gives_the_default_streams_bytes(kind):
    """Fixed frames, plan and maps: only this project's calls run under the stream (the transform, the criterion forward and backward)."""
    data = R.loop_batches(kind, empty=False)
    k = max(range(R.T), key=lambda t: int(data[t]["plan"].n_place.max()) * 100 + int(data[t]["count"].sum()))
    run = cl.augment_batch if kind == "augment" else cl.warp_batch
    with_ids = kind == "warp"
    leaf = fixed_maps(R.D if with_ids else 0)
    reid = reid_criterion() if with_ids else None
    criterion = cl.TrackingLoss(R.DETECTION, reid).train() if with_ids else cl.DetectionLoss(**R.DETECTION)
    frames = device_frames(data[k]["frames"])
    start = {n: v.clone() for n, v in reid.state_dict().items()} if with_ids else None
    torch.cuda.synchronize()

    def once():
        if with_ids:
            reid.load_state_dict(start)
            reid.zero_grad(set_to_none=True)
        v, maps = leaf()
        canvas, targets = run(frames, data[k]["plan"], R.step_targets(k, with_ids))
        out = criterion(maps, targets)
        out["total"].backward()
        res = [canvas] + [targets[n] for n in sorted(targets)] + [out[n] for n in sorted(out)] + [v.grad]
        if with_ids:
            res += [tensor_of(reid, n).grad for n in R.PARAMS] + [tensor_of(reid, n) for n in R.STATS]
        return [t.detach().clone() for t in res]

    first = once()
    torch.cuda.synchronize()
    check_batch(kind, data[k]["plan"], first[0], dict(zip(sorted(["boxes", "labels", "count"] + (["ids"] if with_ids else [])), first[1:])), data[k])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = once()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    third = once()
    torch.cuda.synchronize()
    assert len(first) == len(second) == len(third)
    for n, (a, b, c) in enumerate(zip(first, second, third)):
        assert same_bits(a, b), ("side stream", n)
        assert same_bits(a, c), ("default stream again", n)
