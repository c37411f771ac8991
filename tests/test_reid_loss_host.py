"""CPU: the rule of the re-ID loss (tests/reid_loss_ref.py) against the reference's recorded value, autograd gradients and BatchNorm buffers
(tests/golden/reid_loss_*.npz, written by tools/make_golden_reid_loss.py), the rule's details, the argument checks of loss.reid_loss / reid_loss_grad /
ReIDLoss / TrackingLoss (all raise before any launch), the C ABI's four new symbols, ReIDLoss's state_dict keys, formats.reid_classifier_state and
model.tracking_criterion."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl
import reid_loss_ref as ref
from centernet_lightning_amd import _lib, formats, loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reid_loss_*.npz")))
NAMES = [os.path.basename(p)[10:-4] for p in GOLDEN]
REFERENCE_KEYS = ["classifier.0.weight", "classifier.1.weight", "classifier.1.bias", "classifier.1.running_mean", "classifier.1.running_var",
                  "classifier.1.num_batches_tracked", "classifier.3.weight", "classifier.3.bias"]      # EmbeddingHead.classifier, models/fairmot.py:27-32


def load(path):
    z = np.load(path)
    return z, {k: z[k] for k in ref.KEYS}, json.loads(str(z["settings"]))


def test_fixtures_cover_the_cases_the_issue_names():
    assert set(NAMES) == {"full", "padded", "shared_cell", "origin", "eval"}
    seen = {n: load(p) for n, p in zip(NAMES, GOLDEN)}
    for name, (z, cls, st) in seen.items():
        assert float(z["tol64"]) == float(seen["full"][0]["tol64"]) and 0 < float(z["tol64"]) < 1e-12
        assert os.path.getsize(GOLDEN[NAMES.index(name)]) < 64 * 1024
        assert z["reid"].dtype == np.float32 and all(v.dtype == np.float32 for v in cls.values())
        assert all(z["d_" + k].dtype == np.float64 for k in ref.GRADS) and z["d_reid"].shape == z["reid"].shape
    G = lambda n: seen[n][0]["ids"].shape[1]
    assert all((seen[n][0]["count"] == G(n)).all() for n in ("full", "shared_cell"))
    assert seen["padded"][2]["padded_rows"] and (seen["padded"][0]["count"] < G("padded")).any() and seen["padded"][2]["training"]
    assert not seen["eval"][2]["training"]
    z, _, st = seen["shared_cell"]
    state, x, y, _ = ref.rows_of(z["boxes"], z["ids"], z["count"], *z["reid"].shape[2:], 23, st["stride"])
    assert (x[0, 0], y[0, 0]) == (x[0, 1], y[0, 1])
    z, _, st = seen["origin"]
    state, x, y, _ = ref.rows_of(z["boxes"], z["ids"], z["count"], *z["reid"].shape[2:], 23, st["stride"], padded_rows=True)
    assert state[0, 0] == 2 and (x[0, 0], y[0, 0]) == (0, 0) and (state == 1).sum() >= 2


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_reference(name):
    """The value, the gradients and the running statistics after the step within 4 tol64 of the tensor's largest entry (tol64: the worst deviation the
    generator measured when it wrote the files)."""
    z, cls, st = load(GOLDEN[NAMES.index(name)])
    tol = 4 * float(z["tol64"])
    args = (z["reid"], z["boxes"], z["ids"], z["count"], cls)
    value, grads = ref.reid_loss(*args, **st), ref.reid_loss_grad(*args, **st)
    pairs = [("loss", np.array(value["reid"]), z["loss"]), ("running_mean", value["running_mean64"], z["running_mean_after"]),
             ("running_var", value["running_var64"], z["running_var_after"])] + [("d_" + k, grads[k], z["d_" + k]) for k in ref.GRADS]
    for what, mine, want in pairs:
        assert mine.shape == want.shape, what
        dev = np.abs(mine - want).max() / np.abs(want).max()
        print(name, what, "deviation", dev)
        assert dev <= tol, (what, dev, tol)
    assert not grads["reid"][np.broadcast_to(~grads["read"][:, None], grads["reid"].shape)].any()
    assert value["stepped"] == int(st["training"])


# ----------------------------------------------------------------------------- details of the rule
def small(seed=0, D=6, K=9, H=5, W=7):
    rng = np.random.default_rng(seed)
    reid = rng.normal(0, 1, (2, D, H, W)).astype(np.float32)
    cls = dict(W1=rng.normal(0, 0.5, (D, D)), gamma=rng.uniform(0.5, 1.5, D), beta=rng.normal(0, 0.3, D), running_mean=rng.normal(0, 0.2, D),
               running_var=rng.uniform(0.5, 1.5, D), W2=rng.normal(0, 0.8, (K, D)), b2=rng.normal(0, 0.5, K))
    c = np.array([[[2.7, 1.6], [4.2, 3.9], [0.5, 0.5]], [[5.5, 2.5], [1.1, 4.4], [3.3, 3.3]]]) * 4.0
    boxes = np.concatenate([c - 4.0, np.full_like(c, 8.0)], -1)
    ids = np.array([[0, 3, 5], [8, 1, 2]], np.int64)
    return reid, boxes, ids, np.array([3, 3], np.int32), {k: v.astype(np.float32) for k, v in cls.items()}


def test_trunc_and_round_cells():
    reid, boxes, ids, count, cls = small()
    st_t, xt, yt, _ = ref.rows_of(boxes, ids, count, 5, 7, 9, 4, "trunc")
    st_r, xr, yr, _ = ref.rows_of(boxes, ids, count, 5, 7, 9, 4, "round")
    assert (xt[0, 0], yt[0, 0]) == (2, 1) and (xr[0, 0], yr[0, 0]) == (3, 2)
    assert (xt[1, 0], yt[1, 0]) == (5, 2) and (xr[1, 0], yr[1, 0]) == (6, 2)      # rint: ties to even
    a, b = ref.reid_loss(reid, boxes, ids, count, cls, center="trunc"), ref.reid_loss(reid, boxes, ids, count, cls, center="round")
    assert a["num_rows"] == b["num_rows"] == 6 and a["reid"] != b["reid"]
    # a centre that rounds out of the map is skipped under "round" and kept under "trunc"
    boxes[1, 1, :2] = [6.6 * 4 - 4, 4.7 * 4 - 4]
    assert ref.rows_of(boxes, ids, count, 5, 7, 9, 4, "trunc")[3] == 0 and ref.rows_of(boxes, ids, count, 5, 7, 9, 4, "round")[3] == 1


def test_ignore_index_id_beyond_k_and_padded_rows():
    reid, boxes, ids, count, cls = small()
    base = ref.reid_loss(reid, boxes, ids, count, cls)
    ids2 = ids.copy()
    ids2[0, 1] = -1
    dropped = ref.reid_loss(reid, boxes, ids2, count, cls)
    assert dropped["num_rows"] == 5 and dropped["skipped"] == 0 and dropped["per_row"][0, 1] == 0
    assert ref.reid_loss(reid, boxes, ids2, count, cls, ignore_index=-2)["skipped"] == 1
    ids2[0, 1] = 9
    beyond = ref.reid_loss(reid, boxes, ids2, count, cls)
    assert beyond["num_rows"] == 5 and beyond["skipped"] == 1
    # the dropped row leaves the statistics too: the same value as the batch without it
    ids2[0, 1] = -1
    keep = np.array([0, 2, 1])
    without = ref.reid_loss(reid, np.stack([boxes[0, keep], boxes[1]]), np.stack([ids[0, keep], ids[1]]), np.array([2, 3], np.int32), cls)
    assert without["num_rows"] == 5 and without["reid"] == dropped["reid"]
    # padded rows change the batch statistics (training) and nothing in eval mode
    short = np.array([3, 1], np.int32)
    assert ref.reid_loss(reid, boxes, ids, short, cls, padded_rows=True)["reid"] != ref.reid_loss(reid, boxes, ids, short, cls)["reid"]
    assert ref.reid_loss(reid, boxes, ids, short, cls, padded_rows=True, training=False)["reid"] == ref.reid_loss(reid, boxes, ids, short, cls, training=False)["reid"]
    g = ref.reid_loss_grad(reid, boxes, ids, short, cls, padded_rows=True)
    assert g["read"][1, 0, 0] and g["reid"][1, :, 0, 0].any()          # the padded rows' cell receives a gradient through the statistics
    assert base["stepped"] == 1


def test_fewer_than_two_stat_rows():
    reid, boxes, ids, count, cls = small()
    one = np.array([1, 0], np.int32)
    v, g = ref.reid_loss(reid, boxes, ids, one, cls), ref.reid_loss_grad(reid, boxes, ids, one, cls)
    assert v["reid"] == 0.0 and not v["per_row"].any() and v["stepped"] == 0 and v["num_rows"] == 1
    assert np.array_equal(v["running_mean64"], cls["running_mean"].astype(np.float64)) and np.array_equal(v["running_var64"], cls["running_var"].astype(np.float64))
    assert all(not g[k].any() for k in ref.GRADS)
    e = ref.reid_loss(reid, boxes, ids, one, cls, training=False)
    assert e["reid"] > 0 and e["num_rows"] == 1
    assert ref.reid_loss(reid, boxes, ids, one, cls, padded_rows=True)["reid"] > 0      # the padded rows make a batch


def test_restatement_against_central_differences():
    reid, boxes, ids, count, cls = small(3)
    q = lambda a: (np.round(a * 1024) / 1024).astype(np.float32)
    x0 = {"reid": q(reid), **{k: q(cls[k]) for k in ("W1", "gamma", "beta", "W2", "b2")}}
    rng = np.random.default_rng(1)
    d = {k: rng.choice([-1.0, 1.0], v.shape).astype(np.float32) for k, v in x0.items()}
    h = 2.0 ** -10
    for training, padded in ((True, False), (True, True), (False, False)):
        kw = dict(training=training, padded_rows=padded)
        c = np.array([3, 2], np.int32)
        f = lambda s: ref.reid_loss(x0["reid"] + np.float32(s * h) * d["reid"], boxes, ids, c,
                                    {**{k: x0[k] + np.float32(s * h) * d[k] for k in d if k != "reid"}, "running_mean": cls["running_mean"], "running_var": cls["running_var"]},
                                    **kw)["reid"]
        g = ref.reid_loss_grad(x0["reid"], boxes, ids, c, {**{k: x0[k] for k in d if k != "reid"}, "running_mean": cls["running_mean"], "running_var": cls["running_var"]}, **kw)
        dot = sum(float((g[k] * d[k]).sum()) for k in d)
        np.testing.assert_allclose((f(1) - f(-1)) / (2 * h), dot, rtol=1e-4)


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    for name in ("cnl_reid_loss_workspace_bytes", "cnl_reid_loss_f64", "cnl_reid_loss_grad_workspace_bytes", "cnl_reid_loss_grad_f32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.cnl_version() == _lib.ABI_VERSION == 13
    assert lib.cnl_sizeof_params(5) == ctypes.sizeof(_lib.ReidLossParams) == 48
    assert 0 < lib.cnl_reid_loss_workspace_bytes(3, 5, 64) < lib.cnl_reid_loss_grad_workspace_bytes(3, 5, 64)
    assert lib.cnl_reid_loss_grad_workspace_bytes(3, 5, 64) - lib.cnl_reid_loss_workspace_bytes(3, 5, 64) == 2 * 15 * 64 * 8      # dZ / dH and dE
    for fn in (lib.cnl_reid_loss_workspace_bytes, lib.cnl_reid_loss_grad_workspace_bytes):
        assert fn(1, 1025, 64) == 0 and fn(1, 0, 64) == 0 and fn(1, 1, 257) == 0 and fn(1, 1, 0) == 0 and fn((1 << 16) + 1, 1, 8) == 0
        assert fn(1, 1024, 256) > 0


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    A = 1 << 20                                               # a well aligned address that is never read: every call below is refused before a launch

    def call(grad, p=None, **kw):
        p = loss.reid_params() if p is None else p
        a = dict(reid=A, N=1, D=8, H=4, W=4, boxes=A, ids=A, count=A, Gmax=1, K=5, ws=A, ws_bytes=0)
        a.update(kw)
        common = (a["reid"], 128, 1, 32, 8, a["N"], a["D"], a["H"], a["W"], a["boxes"], a["ids"], a["count"], a["Gmax"], A, A, A, A, A, A, A, a["K"],
                  ctypes.byref(p))
        if grad:
            return lib.cnl_reid_loss_grad_f32(*common, None, A, 128, 1, 32, 8, A, A, A, A, A, A, a["ws"], a["ws_bytes"], None)
        return lib.cnl_reid_loss_f64(*common, A, A, A, A, a["ws"], a["ws_bytes"], None)

    for grad in (False, True):
        assert call(grad) == _lib.CNL_E_WORKSPACE
        for bad in (dict(D=0), dict(D=257), dict(K=1), dict(K=(1 << 20) + 1), dict(Gmax=0), dict(Gmax=1025), dict(H=0), dict(W=(1 << 15) + 1), dict(N=-1),
                    dict(reid=None), dict(boxes=A + 4), dict(ws=A + 8), dict(ids=None)):
            assert call(grad, **bad) == _lib.CNL_E_BAD_ARG, bad
        for field, value in (("stride", 0.0), ("bn_eps", 0.0), ("momentum", 1.5), ("center", 2), ("training", 3)):
            p = loss.reid_params()
            setattr(p, field, value)
            assert call(grad, p=p) == _lib.CNL_E_BAD_ARG, field
        assert call(grad, N=0) == 0                           # an empty batch: nothing to do


# ----------------------------------------------------------------------------- the Python surface
def cpu_classifier(D=8, K=5):
    return dict(W1=torch.zeros(D, D), gamma=torch.ones(D), beta=torch.zeros(D), running_mean=torch.zeros(D), running_var=torch.ones(D), W2=torch.zeros(K, D),
                b2=torch.zeros(K))


def test_argument_checks_raise_before_any_launch():
    reid = torch.zeros(1, 8, 4, 4)
    host = [{"boxes": [[4.0, 4.0, 4.0, 4.0]], "ids": [1]}]
    for fn in (cl.reid_loss, cl.reid_loss_grad):
        with pytest.raises(ValueError, match="center"):
            fn(reid, host, cpu_classifier(), center="floor")
        with pytest.raises(ValueError, match="ignore_index"):
            fn(reid, host, cpu_classifier(), ignore_index=1.5)
        with pytest.raises(ValueError, match="lacks"):
            fn(reid, host, {"W1": torch.zeros(8, 8)})
        with pytest.raises(ValueError, match="float32"):
            fn(reid, host, {**cpu_classifier(), "W2": torch.zeros(5, 8, dtype=torch.float64)})
        with pytest.raises(ValueError, match="gamma"):
            fn(reid, host, {**cpu_classifier(), "gamma": torch.ones(7)})
        with pytest.raises(ValueError, match="channels"):
            fn(torch.zeros(1, 6, 4, 4), host, cpu_classifier())
        with pytest.raises(ValueError, match="float32 tensor"):
            fn(reid.double(), host, cpu_classifier())
        with pytest.raises(ValueError, match="classifier must be"):
            fn(reid, host, torch.nn.Linear(8, 5))
        with pytest.raises(ValueError, match="momentum"):
            fn(reid, host, {**cpu_classifier(), "momentum": None})
        with pytest.raises(RuntimeError, match="HIP devices only"):
            fn(reid, host, cpu_classifier())                  # everything is in order but the device
    with pytest.raises(ValueError, match="want"):
        cl.reid_loss_grad(reid, host, cpu_classifier(), want=("reid", "running_mean"))
    with pytest.raises(ValueError, match="D = 300"):
        cl.reid_loss(torch.zeros(1, 300, 4, 4), host, cpu_classifier(300))
    with pytest.raises(ValueError, match="unknown settings"):
        cl.ReIDLoss(8, 5, box_loss="giou")
    with pytest.raises(ValueError, match="max_track_ids"):
        cl.ReIDLoss(8, 1)
    with pytest.raises(ValueError, match="emb_dim"):
        cl.ReIDLoss(257, 5)
    with pytest.raises(ValueError, match="must be a ReIDLoss"):
        cl.TrackingLoss({}, torch.nn.Identity())
    with pytest.raises(ValueError, match="'reid'"):
        cl.ReIDLoss(8, 5)({"heatmap": reid}, host)


def test_host_targets_are_checked_like_the_detection_targets():
    what = "reid_loss"
    ok = [{"boxes": [[4.0, 4.0, 4.0, 4.0]], "ids": [1]}, {"boxes": np.zeros((0, 4)), "ids": []}]
    _, (boxes, ids, count), G = loss._reid_targets(ok, 2, 4, 4, 5, 4.0, "trunc", -1, what)
    assert G == 1 and count.tolist() == [1, 0] and ids.dtype == np.int64 and boxes.shape == (2, 1, 4)
    for bad, msg in (([{"boxes": [[4.0, 4.0, 4.0, 4.0]], "ids": [5]}, ok[1]], "cannot be a row"),             # id >= K
                     ([{"boxes": [[40.0, 4.0, 4.0, 4.0]], "ids": [1]}, ok[1]], "cannot be a row"),            # cell outside the map
                     ([{"boxes": [[4.0, 4.0, -1.0, 4.0]], "ids": [1]}, ok[1]], "cannot be a row"),
                     ([{"boxes": [[4.0, 4.0, 4.0, 4.0]], "ids": [1, 2]}, ok[1]], "expected"),
                     ([{"boxes": [[4.0, 4.0, 4.0, 4.0]]}, ok[1]], "'boxes', 'ids'"),
                     (ok[:1], "2 images")):
        with pytest.raises(ValueError, match=msg):
            loss._reid_targets(bad, 2, 4, 4, 5, 4.0, "trunc", -1, what)
    # a box without identity is no error, whatever its numbers
    _, (_, ids, count), _ = loss._reid_targets([{"boxes": [[400.0, 4.0, 4.0, 4.0]], "ids": [-1]}, ok[1]], 2, 4, 4, 5, 4.0, "trunc", -1, what)
    assert ids[0, 0] == -1 and count[0] == 1
    # (15.9 / 4 truncs inside a 4-wide map and rounds out of it)
    edge = [{"boxes": [[13.9, 4.0, 4.0, 4.0]], "ids": [1]}, ok[1]]
    loss._reid_targets(edge, 2, 4, 4, 5, 4.0, "trunc", -1, what)
    with pytest.raises(ValueError, match="cannot be a row"):
        loss._reid_targets(edge, 2, 4, 4, 5, 4.0, "round", -1, what)
    for bad in ({"boxes": torch.zeros(2, 1, 4), "ids": torch.zeros(2, 1, dtype=torch.int64), "count": torch.zeros(2, dtype=torch.int32)},      # float32 boxes
                {"boxes": torch.zeros(2, 1, 4, dtype=torch.float64), "count": torch.zeros(2, dtype=torch.int32)}):
        with pytest.raises(ValueError):
            loss._reid_targets(bad, 2, 4, 4, 5, 4.0, "trunc", -1, what)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        loss._reid_targets({"boxes": torch.zeros(2, 1, 4, dtype=torch.float64), "ids": torch.zeros(2, 1, dtype=torch.int64),
                            "count": torch.zeros(2, dtype=torch.int32)}, 2, 4, 4, 5, 4.0, "trunc", -1, what)


def test_reid_loss_module_has_the_reference_keys():
    m = cl.ReIDLoss()
    assert list(m.state_dict()) == REFERENCE_KEYS
    assert tuple(m.classifier[0].weight.shape) == (64, 64) and m.classifier[0].bias is None and tuple(m.classifier[3].weight.shape) == (1000, 64)
    assert isinstance(m.classifier[1], torch.nn.BatchNorm1d) and isinstance(m.classifier[2], torch.nn.ReLU) and m.loss_weight == 1.0
    assert m.training and not m.eval().training


def test_reid_classifier_state_round_trips_a_checkpoint():
    z, cls, _ = load(GOLDEN[NAMES.index("full")])
    D, K = cls["W1"].shape[0], cls["W2"].shape[0]
    prefix = "model.output_heads.reid."
    ckpt = {"state_dict": {prefix + "classifier.0.weight": torch.from_numpy(cls["W1"]), prefix + "classifier.1.weight": torch.from_numpy(cls["gamma"]),
                           prefix + "classifier.1.bias": torch.from_numpy(cls["beta"]), prefix + "classifier.1.running_mean": torch.from_numpy(cls["running_mean"]),
                           prefix + "classifier.1.running_var": torch.from_numpy(cls["running_var"]), prefix + "classifier.1.num_batches_tracked": torch.tensor(7),
                           prefix + "classifier.3.weight": torch.from_numpy(cls["W2"]), prefix + "classifier.3.bias": torch.from_numpy(cls["b2"]),
                           prefix + "head.0.weight": torch.zeros(3), "model.backbone.conv1.weight": torch.zeros(3)}}
    state = formats.reid_classifier_state(ckpt)
    assert list(state) == REFERENCE_KEYS
    m = cl.ReIDLoss(D, K)
    m.load_state_dict(state)                                  # strict
    t, eps, momentum, steps = loss._classifier(m, "test")
    for k in ref.KEYS:
        assert np.array_equal(t[k].detach().numpy(), cls[k]), k
    assert int(steps) == 7 and eps == 1e-5 and momentum == 0.1
    assert list(formats.reid_classifier_state(ckpt["state_dict"])) == REFERENCE_KEYS      # a bare state_dict too
    assert all(formats.is_training_only_key(k) == (".classifier." in k) for k in ckpt["state_dict"])      # the model loader keeps skipping them
    with pytest.raises(ValueError, match="no '<head>.classifier"):
        formats.reid_classifier_state({"model.backbone.conv1.weight": torch.zeros(3)})


def test_tracking_criterion_reads_the_reid_head():
    tracking = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "tracking_resnet34_fpn.yaml"))
    crit = tracking.tracking_criterion()
    assert isinstance(crit, cl.TrackingLoss) and isinstance(crit.reid, cl.ReIDLoss) and isinstance(crit.detection, cl.DetectionLoss)
    assert (crit.reid.emb_dim, crit.reid.max_track_ids, crit.reid.loss_weight) == (64, 800, 1.0) and crit.reid.settings == {"stride": tracking.stride}
    assert crit.detection.settings == tracking.criterion().settings
    assert tracking.tracking_criterion(max_track_ids=14455).reid.max_track_ids == 14455
    assert isinstance(tracking.criterion(), cl.DetectionLoss)                    # unchanged
    detection = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet34_fpn.yaml"))
    with pytest.raises(ValueError, match="tracking model"):
        detection.tracking_criterion()
