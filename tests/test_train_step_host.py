"""No GPU: the float64 twin of whole training steps (tests/train_step_ref.py) judged on its own.  It learns; the fp32 host loop's distance from it
(the yardstick of tests/test_gpu_train_step.py's trajectory bound) is printed; three planted errors of the kind a user cannot see each move the
final state at least ten times past that bound; and a loss scale of 2^k scales the twin's float64 gradients exactly.

The plan seeds and the learning rate of train_step_ref were chosen here, on the twin alone, for two things: a detection total that falls at every
step with room (without the empty step: a step without boxes is a sum over the whole map divided by max(1, 0)), and fp32 host loops that stay a
few ulps' worth away from the twin (a ReLU or the decode's clamp changing sides between the two moves a loop by 1e-5 at once: such a seed would
make the bound say little, which the planted errors below would show)."""
import copy

import numpy as np
import torch

import train_step_ref as R


def totals(loop):
    return [float(v["total"]) for v in loop["losses"]]


# ----------------------------------------------------------------------------- the twin learns
def test_the_detection_twin_learns_at_every_step():
    run = R.detection_loop(torch.float64, empty_step=None)
    seen = totals(run)
    print("float64 detection totals", [round(v, 4) for v in seen], "fall %.1f %%" % (100 * (1 - seen[-1] / seen[0])))
    assert len(seen) == R.T == 8 and all(b < a for a, b in zip(seen, seen[1:])), seen
    assert seen[-1] <= 0.98 * seen[0]
    assert all(v["skipped"] == 0 for v in run["losses"])


def test_the_tracking_twin_learns_and_always_has_two_rows():
    twin, _ = R.reference_loops("warp")
    seen = totals(twin)
    print("float64 tracking totals", [round(v, 4) for v in seen], "reid", [round(float(v["reid"]), 4) for v in twin["losses"]], "rows",
          [v["num_rows"] for v in twin["losses"]])
    assert seen[-1] < seen[0]
    assert all(v["num_rows"] >= 2 and v["skipped"] == 0 and v["reid_skipped"] == 0 for v in twin["losses"])
    assert twin["num_batches_tracked"] == R.T
    data = R.loop_batches("warp")
    assert any((b["ids"] == -1).any() for b in data) and any(a["boxes"].shape[1] > b["boxes"].shape[1] for a, b in zip(data, data[1:]))


def test_the_batches_have_the_cases_the_device_test_is_about():
    data = R.loop_batches("augment")
    counts, slots = [int(b["count"].sum()) for b in data], [b["boxes"].shape[1] for b in data]
    print("boxes per step", counts, "target slots per image", slots, "placements", [b["plan"].n_place.tolist() for b in data])
    assert counts[R.EMPTY_STEP] == 0 and all(c > 0 for t, c in enumerate(counts) if t != R.EMPTY_STEP)
    assert any(a > b for a, b in zip(slots, slots[1:])) and any(a < b for a, b in zip(slots, slots[1:]))
    assert {1, 4} <= {int(k) for b in data for k in b["plan"].n_place}
    assert any(f == 2 for b in data for f in b["frames"]) and R.FRAME_BOXES[2] == 0 and max(R.FRAME_BOXES) == 12


# ----------------------------------------------------------------------------- the yardstick
def yardstick(kind):
    twin, yard = R.reference_loops(kind)
    return R.distance(yard["params"], twin["params"]), R.loss_gaps(yard["losses"], twin["losses"])


def test_the_fp32_host_loops_stay_close_to_the_twin():
    for kind in ("augment", "warp"):
        d32, gaps = yardstick(kind)
        print(f"{kind}: d32 {d32:.3e}, bound {R.bound(d32):.3e}; relative loss gaps per step {[f'{g:.1e}' for g in gaps]}, bound {R.bound(max(gaps)):.3e}")
        assert 0 < d32 < np.inf and np.isfinite(gaps).all()          # (a yardstick that a changed branch made large shows in the planted errors below)


# ----------------------------------------------------------------------------- the criterion would notice
def scaled_box_gradient(t, grads, loss):
    grads["box_2d"] *= 1.0 + 1e-3


def dropped_image(t, grads, loss):
    if t == 3:
        grads["heatmap"][1] = 0.0


def test_a_planted_error_moves_the_detection_loop_ten_bounds_away():
    twin, _ = R.reference_loops("augment")
    d32, _ = yardstick("augment")
    for name, tamper in (("box gradient x (1 + 1e-3)", scaled_box_gradient), ("one image's heatmap gradient dropped at step 3", dropped_image)):
        moved = R.distance(R.detection_loop(torch.float64, tamper=tamper)["params"], twin["params"])
        print(f"{name}: moved {moved:.3e}, bound {R.bound(d32):.3e}, ratio {moved / R.bound(d32):.1f}")
        assert moved >= 10 * R.bound(d32), name


def test_a_planted_error_moves_the_tracking_loop_ten_bounds_away():
    twin, yard = R.reference_loops("warp")
    d32, _ = yardstick("warp")
    s32 = R.distance(yard["stats"][-1], twin["stats"][-1])
    wrong = R.tracking_loop(torch.float64, momentum=0.11)
    moved = R.distance(wrong["stats"][-1], twin["stats"][-1])
    print(f"running statistics stepped with momentum 0.11: moved {moved:.3e}, bound {R.bound(s32):.3e}, ratio {moved / R.bound(s32):.1f}")
    assert moved >= 10 * R.bound(s32)
    assert R.distance(wrong["params"], twin["params"]) == 0.0          # (training reads the batch statistics: only the buffers can show it)
    moved = R.distance(R.tracking_loop(torch.float64, tamper=scaled_box_gradient)["params"], twin["params"])
    print(f"box gradient x (1 + 1e-3): moved {moved:.3e}, bound {R.bound(d32):.3e}, ratio {moved / R.bound(d32):.1f}")
    assert moved >= 10 * R.bound(d32)


# ----------------------------------------------------------------------------- exact scaling
def test_a_power_of_two_scale_scales_the_twins_gradients_exactly():
    batch = R.loop_batches("warp")[0]
    model, classifier = R.TinyNet(R.C, R.D).double(), R.Classifier(torch.float64)

    def grads(scale):
        m, c = copy.deepcopy(model), copy.deepcopy(classifier)
        optimiser = torch.optim.SGD(list(m.parameters()) + list(c.parameters()), lr=R.LR, momentum=R.MOMENTUM)
        return R.step(m, optimiser, batch["canvas"], batch, R.DETECTION, c, scale=scale)[1]

    plain = grads(1.0)
    assert all(np.abs(v).max() > 0 for v in plain.values())
    for k in (10, -3):
        scaled = grads(2.0 ** k)
        for name in plain:
            assert np.array_equal(scaled[name], plain[name] * 2.0 ** k), (k, name)
