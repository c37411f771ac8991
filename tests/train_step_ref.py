"""Whole training steps restated on the CPU: the float64 twin of a loop that joins TrainAugment / TrainWarp, a small torch model, DetectionLoss /
TrackingLoss and torch.optim.SGD.  A plain helper (no tests) for tests/test_train_step_host.py and tests/test_gpu_train_step.py.  There is no new
loss mathematics here: a step is put together from tests/loss_ref.py, loss_grad_ref.py, reid_loss_ref.py, augment_ref.py and warp_ref.py.

    canvas (uint8, expected_canvas of the step's plan)  ->  TinyNet in its own dtype  ->  maps rounded to fp32  ->  the restated loss and its float64
    map gradients  ->  torch.autograd.backward(maps, grads)  ->  the classifier's gradients and running statistics from the restatement  ->  SGD

detection_loop / tracking_loop(torch.float64, ...) is the twin; the same loop with torch.float32 is the yardstick: only the model's arithmetic (and
the stored parameters) are fp32 there, so its distance from the twin is what fp32 rounding accumulated over T steps amounts to on this problem.
Everything that is drawn is drawn from fixed seeds: frames, source targets, the model, the classifier, and the plans (cl.sample_augment /
cl.sample_warp with numpy's default_rng(seed), which is what TrainAugment(seed=seed) / TrainWarp(seed=seed) draw on the host)."""
import functools

import numpy as np
import torch

import augment_ref
import loss_grad_ref
import loss_ref
import reid_loss_ref
import warp_ref
import centernet_lightning_amd as cl

HEIGHT, WIDTH, STRIDE = 64, 160, 4            # a 16 x 40 map: two 8-row tile rows, two 32-column tiles, the second one partial
MAP_H, MAP_W = 16, 40
FRAME_SIZES = [(37, 53), (120, 200), (64, 48), (90, 160), (33, 70), (64, 64)]
FRAME_BOXES = [5, 12, 0, 7, 3, 9]             # source boxes per frame: one frame has none
N, C, D, K, T = 4, 3, 8, 20, 8
EMPTY_STEP = 5                                # the detection loop's step without a box in any image (the tracking loop has none: it needs two rows)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DETECTION = dict(stride=STRIDE, box_loss="giou", box_loss_weight=5.0)
REID_WEIGHT, BN_MOMENTUM, BN_EPS = 0.7, 0.1, 1e-5
LR, MOMENTUM = 0.05, 0.9
HEAD_GAIN = 0.5                               # of the head's drawn weights: first-step logits stay near the bias
AUGMENT = dict(mosaic=0.5, flip=0.5, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, cutout=(2, 12, 20))
WARP = dict(rotate=15.0, affine_scale=(0.8, 1.25), shear=8.0, mosaic=0.5, flip=0.5, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1,
            cutout=(2, 12, 20))
SEEDS = {"augment": 29, "warp": 11}        # of the plans: chosen on the twin alone (tests/test_train_step_host.py says for what)
MARGIN = 4.0
PARAMS = ("W1", "gamma", "beta", "W2", "b2")                 # the classifier's trainable tensors, by reid_loss_ref's names
STATS = ("running_mean", "running_var")


# ----------------------------------------------------------------------------- the data
@functools.lru_cache(maxsize=None)
def frames():
    """The six source frames, uint8 [h, w, 3]: blocks of colour under noise, so that a crop, a flip and a turn all change the canvas."""
    rng = np.random.default_rng(101)
    out = []
    for (h, w) in FRAME_SIZES:
        coarse = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3))
        img = np.kron(coarse, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(-24, 25, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def source_targets():
    """Per frame {"boxes" [m, 4] x y w h inside the frame, "labels" [m], "ids" [m]}: 0 to 12 boxes, identities 0..K-1, three of them -1."""
    rng = np.random.default_rng(202)
    out, next_id = [], 0
    for (h, w), m in zip(FRAME_SIZES, FRAME_BOXES):
        size = rng.uniform(0.2, 0.6, (m, 2)) * (w, h)
        corner = rng.uniform(0.0, 1.0, (m, 2)) * ((w, h) - size)
        ids = (np.arange(m) + next_id) % K
        next_id += m
        out.append({"boxes": np.concatenate([corner, size], 1).astype(np.float64), "labels": rng.integers(0, C, m).astype(np.int64), "ids": ids.astype(np.int64)})
    for f, j in ((0, 1), (1, 4), (5, 0)):
        out[f]["ids"][j] = -1
    return out


def step_frames(t):
    """The four frames of step t: a window that moves over the six, so the sizes, the counts and Gmax change from step to step (Gmax: 12, 12, 9, 9, 12, ...)."""
    return [(t + i) % len(FRAME_SIZES) for i in range(N)]


def step_targets(t, with_ids, empty_step=None):
    """The host list TrainAugment / TrainWarp takes at step t."""
    keys = ("boxes", "labels", "ids") if with_ids else ("boxes", "labels")
    src = source_targets()
    return [{k: (src[f][k][:0] if t == empty_step else src[f][k]) for k in keys} for f in step_frames(t)]


def pad_list(items):
    """The host list zero-padded as the package pads it: boxes [F, Gmax, 4], labels, ids (or None), count, Gmax = max(1, most boxes)."""
    G = max([1] + [len(d["labels"]) for d in items])
    boxes, labels, count = np.zeros((len(items), G, 4)), np.zeros((len(items), G), np.int64), np.array([len(d["labels"]) for d in items], np.int32)
    ids = np.zeros((len(items), G), np.int64) if "ids" in items[0] else None
    for n, d in enumerate(items):
        boxes[n, :count[n]], labels[n, :count[n]] = d["boxes"], d["labels"]
        if ids is not None:
            ids[n, :count[n]] = d["ids"]
    return boxes, labels, ids, count


@functools.lru_cache(maxsize=None)
def batches(kind, steps=T, seed=None, empty_step=None):
    """The batches of a loop, step by step: kind "augment" (sample_augment, AUGMENT) or "warp" (sample_warp, WARP, targets with ids).
    -> [{"frames": indices, "plan", "canvas" uint8 [N, 64, 160, 3], "boxes" [N, Gout, 4] f64, "labels", "ids" or None, "count"}], never to be written to."""
    rng = np.random.default_rng(SEEDS[kind] if seed is None else seed)
    sample, settings, ref = (cl.sample_augment, AUGMENT, augment_ref) if kind == "augment" else (cl.sample_warp, WARP, warp_ref)
    out = []
    for t in range(steps):
        idx = step_frames(t)
        plan = sample([FRAME_SIZES[f] for f in idx], HEIGHT, WIDTH, rng, **settings).check()
        boxes, labels, ids, count = pad_list(step_targets(t, kind == "warp", empty_step))
        ob, ol, oi, oc = ref.expected_boxes(plan, boxes, labels, ids, count)
        out.append({"frames": idx, "plan": plan, "canvas": ref.expected_canvas([frames()[f] for f in idx], plan), "boxes": ob, "labels": ol, "ids": oi, "count": oc})
    return out


# ----------------------------------------------------------------------------- the model
class TinyNet(torch.nn.Module):
    """Stands in for the model: stem Conv2d(3, 16, 3, stride 4) + ReLU, Conv2d(16, 16, 3) + ReLU, head Conv2d(16, C + 4 [+ D], 1).  The outputs are
    channel slices of the head's one tensor (non-contiguous views, as from a real head); the heatmap bias is -2.19; the box bias puts most box
    outputs above 0 and some below.  Its fp32 values are drawn from `seed` on the host whatever dtype and device it is moved to afterwards."""

    def __init__(self, classes=C, emb=0, seed=3):
        super().__init__()
        self.classes, self.emb = classes, emb
        self.stem = torch.nn.Conv2d(3, 16, 3, stride=STRIDE, padding=1)
        self.middle = torch.nn.Conv2d(16, 16, 3, padding=1)
        self.head = torch.nn.Conv2d(16, classes + 4 + emb, 1)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for conv in (self.stem, self.middle, self.head):
                fan_in = conv.weight[0].numel()
                conv.weight.copy_((torch.rand(conv.weight.shape, generator=g) * 2 - 1) * (3.0 / fan_in) ** 0.5)
                conv.bias.copy_((torch.rand(conv.bias.shape, generator=g) * 2 - 1) * 0.1)
            self.head.weight *= HEAD_GAIN
            self.head.bias[:classes] = -2.19
            self.head.bias[classes:classes + 4] += 1.0
        self.register_buffer("mean", torch.tensor(MEAN).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor(STD).view(1, 3, 1, 1))

    def forward(self, canvas_u8):
        """canvas uint8 [N, H, W, 3] -> ({"heatmap", "box_2d"[, "reid"]}: channel slices, the head's tensor)"""
        x = canvas_u8.permute(0, 3, 1, 2).to(self.mean.dtype) / 255.0
        x = (x - self.mean) / self.std
        y = self.head(torch.relu(self.middle(torch.relu(self.stem(x)))))
        c = self.classes
        maps = {"heatmap": y[:, :c], "box_2d": y[:, c:c + 4]}
        if self.emb:
            maps["reid"] = y[:, c + 4:]
        return maps, y


def classifier_values(emb=D, ids=K, seed=5):
    """The re-ID classifier's seven tensors as fp32 numpy, by reid_loss_ref.KEYS: torch's initial statistics, drawn weights."""
    rng = np.random.default_rng(seed)
    v = dict(W1=rng.uniform(-1, 1, (emb, emb)) / np.sqrt(emb), gamma=rng.uniform(0.8, 1.2, emb), beta=rng.uniform(-0.1, 0.1, emb), running_mean=np.zeros(emb),
             running_var=np.ones(emb), W2=rng.uniform(-1, 1, (ids, emb)) / np.sqrt(emb), b2=rng.uniform(-0.1, 0.1, ids))
    return {k: a.astype(np.float32) for k, a in v.items()}


class Classifier(torch.nn.Module):
    """The classifier's tensors on the host, in the loop's dtype: five parameters the optimiser steps, two statistics and the step count."""

    def __init__(self, dtype, values=None):
        super().__init__()
        values = classifier_values() if values is None else values
        for k in PARAMS:
            setattr(self, k, torch.nn.Parameter(torch.from_numpy(values[k]).to(dtype)))
        for k in STATS:
            self.register_buffer(k, torch.from_numpy(values[k]).to(dtype))
        self.num_batches_tracked = 0

    def numpy(self):
        return {k: getattr(self, k).detach().numpy() for k in reid_loss_ref.KEYS}


# ----------------------------------------------------------------------------- one step
def list_targets(boxes, labels, count):
    return [(boxes[n, :count[n]], labels[n, :count[n]]) for n in range(len(count))]


def rounded(maps):
    """The maps as the criteria read them: fp32 numpy, contiguous."""
    return {k: np.ascontiguousarray(v.detach().to(torch.float32).cpu().numpy()) for k, v in maps.items()}


def step(model, optimiser, canvas_u8, targets, settings, classifier=None, scale=1.0, reid_weight=REID_WEIGHT, momentum=BN_MOMENTUM, tamper=None):
    """One training step on the host.  canvas_u8 [N, H, W, 3] uint8 numpy; targets: {"boxes" [N, G, 4] f64, "labels", "count"[, "ids"]} numpy; settings:
    detection_loss's.  The gradient is that of scale * total, total = heatmap_weight heatmap + box_weight box_2d [+ reid_weight reid].  tamper(grads,
    loss): called on the float64 map gradients before they go back (the host tests plant their errors there).  momentum: of the running statistics.
    -> (the loss dict: "heatmap", "box_2d", "total", "skipped"[, "reid", "num_rows", "correct", "reid_skipped"], {"heatmap", "box_2d"[, "reid"]}
    float64 map gradients[, + the classifier's float64 gradients by name])"""
    optimiser.zero_grad(set_to_none=True)
    maps, _ = model(torch.from_numpy(canvas_u8))
    m32 = rounded(maps)
    tg = list_targets(targets["boxes"], targets["labels"], targets["count"])
    value = loss_ref.detection_loss(m32["heatmap"], m32["box_2d"], tg, **settings)
    grad = loss_grad_ref.detection_loss_grad(m32["heatmap"], m32["box_2d"], tg, heatmap_scale=scale * settings.get("heatmap_loss_weight", 1.0),
                                             box_scale=scale * settings.get("box_loss_weight", 1.0), **settings)
    loss = {k: value[k] for k in ("heatmap", "box_2d", "total", "skipped")}
    grads = {"heatmap": grad["heatmap_grad64"], "box_2d": grad["box_2d_grad64"]}
    if classifier is not None:
        args = (m32["reid"], targets["boxes"], targets["ids"], targets["count"], classifier.numpy())
        kw = dict(training=True, stride=settings.get("stride", 4), bn_eps=BN_EPS, momentum=momentum)
        r = reid_loss_ref.reid_loss(*args, **kw)
        rg = reid_loss_ref.reid_loss_grad(*args, scale=scale * reid_weight, **kw)
        loss.update(reid=r["reid"], num_rows=r["num_rows"], correct=r["correct"], reid_skipped=r["skipped"], total=value["total"] + reid_weight * r["reid"])
        grads["reid"] = rg["reid"]
        grads.update({k: rg[k] for k in PARAMS})
    if tamper is not None:
        tamper(grads, loss)
    names = [k for k in ("heatmap", "box_2d", "reid") if k in maps]
    torch.autograd.backward([maps[k] for k in names], [torch.from_numpy(grads[k]).to(maps[k].dtype) for k in names])
    if classifier is not None:
        with torch.no_grad():
            for k in PARAMS:
                p = getattr(classifier, k)
                p.grad = torch.from_numpy(grads[k]).to(p.dtype)
            classifier.running_mean.copy_(torch.from_numpy(r["running_mean64"]))
            classifier.running_var.copy_(torch.from_numpy(r["running_var64"]))
            classifier.num_batches_tracked += r["stepped"]
    optimiser.step()
    return loss, grads


# ----------------------------------------------------------------------------- the loops
def tensors_of(module):
    return {k: v.detach().to(torch.float64).cpu().numpy().copy() for k, v in module.named_parameters()}


def _loop(kind, dtype, steps, seed, empty_step, lr, tamper, momentum):
    data = batches(kind, steps, seed, empty_step)
    model = TinyNet(C, D if kind == "warp" else 0).to(dtype)
    classifier = Classifier(dtype) if kind == "warp" else None
    params = list(model.parameters()) + (list(classifier.parameters()) if classifier is not None else [])
    optimiser = torch.optim.SGD(params, lr=lr, momentum=MOMENTUM)
    losses, stats = [], []
    for t, b in enumerate(data):
        loss, _ = step(model, optimiser, b["canvas"], b, DETECTION, classifier, momentum=momentum, tamper=None if tamper is None else functools.partial(tamper, t))
        losses.append(loss)
        if classifier is not None:
            stats.append({k: getattr(classifier, k).detach().to(torch.float64).numpy().copy() for k in STATS})
    out = {"losses": losses, "params": tensors_of(model)}
    if classifier is not None:
        out["params"].update({"classifier." + k: v for k, v in tensors_of(classifier).items()})
        out.update(stats=stats, num_batches_tracked=classifier.num_batches_tracked)
    return out


def detection_loop(dtype, steps=T, seed=SEEDS["augment"], empty_step=EMPTY_STEP, lr=LR, tamper=None):
    """`steps` steps of TinyNet(C) under DetectionLoss(giou, box weight 5) and SGD(lr, momentum 0.9) on the "augment" batches.  tamper(t, grads, loss).
    -> {"losses": the loss dict of every step, "params": {name: float64 numpy} after the last step}"""
    return _loop("augment", dtype, steps, seed, empty_step, lr, tamper, BN_MOMENTUM)


def tracking_loop(dtype, steps=T, seed=SEEDS["warp"], lr=LR, tamper=None, momentum=BN_MOMENTUM):
    """`steps` steps of TinyNet(C, D) and the classifier under TrackingLoss(ReIDLoss(D, K, loss_weight 0.7)) on the "warp" batches.
    -> detection_loop's dict with the classifier's parameters under "classifier.", plus "stats": the running statistics after every step, and
    "num_batches_tracked"."""
    return _loop("warp", dtype, steps, seed, None, lr, tamper, momentum)


@functools.lru_cache(maxsize=None)
def reference_loops(kind):
    """(the float64 twin, the fp32 yardstick) of the loop the GPU test runs; shared, never to be written to."""
    loop = detection_loop if kind == "augment" else tracking_loop
    return loop(torch.float64), loop(torch.float32)


def loop_batches(kind, empty=True):
    """The batches reference_loops(kind) ran on (empty=False: the detection loop's without its empty step)."""
    return batches(kind, T, SEEDS[kind], EMPTY_STEP if kind == "augment" and empty else None)


# ----------------------------------------------------------------------------- distances and the bound
def distance(got, twin):
    """max over tensors of max |got - twin| / max |twin|"""
    assert set(got) == set(twin)
    return max(float(np.abs(np.asarray(got[k], np.float64) - twin[k]).max() / np.abs(twin[k]).max()) for k in twin)


def loss_gaps(got, twin, key="total"):
    """Per step |got - twin| / |twin| of one loss."""
    return [abs(float(a[key]) - float(b[key])) / abs(float(b[key])) for a, b in zip(got, twin)]


def bound(yardstick, steps=T):
    """What a correct fp32 run may be away from the twin: MARGIN x max(the fp32 host loop's own distance, steps x 2^-23).  The device's torch
    convolutions sum in another order than the host's, with the same unit roundoff and over the same steps: 4 x covers the order, and the floor of
    one half-ulp per step covers a yardstick that happens to come out luckier than rounding allows on average."""
    return MARGIN * max(float(yardstick), steps * 2.0 ** -23)
