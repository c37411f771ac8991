"""CPU: the shared target reader (_targets.py) driven directly with the column spec of each of its five consumers: what it refuses, with which
exception and words, and what it pads.  The expected exception types and fragments are what the readers each consumer had before (loss._padded_targets,
augment._list_targets / _device_targets, coco_eval._per_image / CocoEvaluator._targets / _detections) raised for the same input: recorded from them,
and every fragment is one their message held too."""
import numpy as np
import pytest
import torch

from centernet_lightning_amd import _targets, augment, coco_eval

N, G = 2, 3
# the spec (_targets.columns: boxes, the columns, count), the rest of read_list's / read_padded's arguments, and the tuple lengths the consumer's is_padded call takes (None: a dict only)
SPECS = {
    "detection_loss": (_targets.LABELS, dict(cap=1024), {}, (3,)),
    "reid_loss": (_targets.IDS, dict(cap=1024), {}, (4,)),
    "augment_batch": (augment._COLUMNS, dict(optional=("ids",)), dict(against="frames"), (3, 4)),
    "coco_targets": (_targets.LABELS, dict(cap=1024), dict(against="detections"), (3,)),
    "coco_preds": (coco_eval._DETECTIONS, dict(cap=1024), dict(arg="preds"), None),
}
PADDED_PREDS = dict(arg="detections", one="detection", dim="k", optional=("count",))


def named(consumer):
    """[(name, numpy dtype)] of the consumer's columns beside the boxes and the count"""
    return [(c.name, c.numpy) for c in SPECS[consumer][0] if c.name not in ("boxes", "count")]


def image(consumer, n, **change):
    """A good per-image dict of n boxes with every column of the consumer (the optional ids left out)."""
    d = {"boxes": np.arange(4 * n, dtype=np.float64).reshape(n, 4)}
    d.update({name: np.arange(n).astype(dtype) for name, dtype in named(consumer) if name != "ids" or consumer == "reid_loss"})
    d.update(change)
    return d


def padded(consumer, **change):
    """A good padded dict of CPU tensors with every column of the consumer (the optional ids left out)."""
    d = {c.name: torch.zeros((N, G, 4)[:c.rank], dtype=c.torch) for c in SPECS[consumer][0] if c.name != "ids" or consumer == "reid_loss"}
    d.update(change)
    return {k: v for k, v in d.items() if v is not None}


def inputs(consumer):
    """case -> the targets a consumer is handed"""
    good, col = [image(consumer, 3), image(consumer, 0)], named(consumer)[0][0]
    other = torch.float32 if SPECS[consumer][0][0].torch != torch.float32 else torch.float64
    four = tuple(padded("reid_loss", labels=torch.zeros((N, G), dtype=torch.int64))[k] for k in _targets.TUPLE)        # (boxes, labels, count, ids)
    return {
        "wrong length": good[:1],
        "an entry that is no dict": [good[0], "image"],
        "a missing key": [good[0], {"boxes": np.zeros((0, 4))}],
        "data that is not numeric": [image(consumer, 3, boxes=[["a"] * 4] * 3), good[1]],
        "boxes that are not [n, 4]": [image(consumer, 3, boxes=np.zeros((3, 3))), good[1]],
        "a column of another length": [image(consumer, 3, **{col: [0, 1]}), good[1]],
        "one box over the cap": [image(consumer, 1025), good[1]],
        "ids in one image only": [image(consumer, 3, ids=[0, 1, 2]), {k: v for k, v in good[1].items() if k != "ids"}],
        "images without boxes": [image(consumer, 0), image(consumer, 0, boxes=[])],
        "padded: a missing key": padded(consumer, count=None),
        "padded: a wrong dtype": padded(consumer, boxes=torch.zeros((N, G, 4), dtype=other)),
        "padded: a wrong rank": padded(consumer, **{col: torch.zeros((N, G, 1), dtype=padded(consumer)[col].dtype)}),
        "padded: a wrong shape": padded(consumer, count=torch.zeros((N + 1,), dtype=torch.int32)),
        "padded: CPU tensors": padded(consumer),
        "padded: a tuple of CPU tensors": four if SPECS[consumer][3] in ((4,), (3, 4)) else four[:3],      # the longest the consumer takes
    }


def read(consumer, targets):
    """What the consumer does with its targets: the form is told apart, then one of the two readers runs with the consumer's spec."""
    columns, common, list_only, lengths = SPECS[consumer]
    n = None if consumer == "coco_preds" else N
    if lengths is None and isinstance(targets, dict):
        return _targets.read_padded(targets, n, columns, consumer, **common, **PADDED_PREDS)
    if lengths is not None and _targets.is_padded(targets, lengths):
        return _targets.read_padded(targets, n, columns, consumer, **common)
    return _targets.read_list(targets, n, columns, consumer, **common, **list_only)


V, R = ValueError, RuntimeError
LIST_FORM = (V, "must be a dict with")              # a tuple the consumer does not take is read as a list of per-image dicts
# case -> what each consumer raises (None: it reads the input), in the order of SPECS
EXPECTED = {
    "wrong length": [(V, "2 images of outputs against 1 of targets"), (V, "2 images"), (V, "against 1"), (V, "2 images of detections against 1 of targets"), None],
    "an entry that is no dict": [(V, "targets[1] must be a dict with 'boxes', 'labels'"), (V, "targets[1] must be a dict with 'boxes', 'ids'"),
                                 (V, "targets[1] must be a dict with 'boxes', 'labels'"), (V, "targets[1] must be a dict with 'boxes', 'labels'"),
                                 (V, "preds[1] must be a dict with 'boxes'")],
    "a missing key": [(V, "targets[1] must be a dict with 'boxes', 'labels'"), (V, "targets[1] must be a dict with 'boxes', 'ids'"),
                      (V, "targets[1] must be a dict with 'boxes', 'labels'"), (V, "targets[1] must be a dict with 'boxes', 'labels'"),
                      (V, "preds[1] must be a dict with 'boxes'")],
    "data that is not numeric": [(V, "is not numeric: could not convert string to float")] * 5,
    "boxes that are not [n, 4]": [(V, "targets[0] has boxes (3, 3)")] * 4 + [(V, "preds[0] has boxes (3, 3)")],
    "a column of another length": [(V, "expected [n, 4] and [n]")] * 4 + [(V, "preds[0] has")],
    "one box over the cap": [(V, "targets[0] has 1025 boxes; at most 1024 per image are supported")] * 2 + [None] +
                            [(V, "targets[0] has 1025 boxes; at most 1024 per image are supported"), (V, "preds[0] has 1025 boxes; at most 1024 per image")],
    "ids in one image only": [None, (V, "targets[1] must be a dict with 'boxes', 'ids'"), (V, "has 'ids' or none has"), None, None],
    "images without boxes": [None] * 5,
    "padded: a missing key": [(V, "device targets need 'boxes'")] * 4 + [(R, "HIP devices only")],        # (the count of the detections is optional)
    "padded: a wrong dtype": [(V, "targets 'boxes' must be torch.float64"), (V, "targets 'boxes' must be torch.float64"), (V, "targets 'boxes' must be"),
                              (V, "targets 'boxes' must be torch.float64"), (V, "boxes' must be torch.float32 with 3 dimensions, got torch.float64 (2, 3, 4)")],
    # augment_batch in the next two: its former reader judged tensor by tensor and met the CPU boxes first (RuntimeError); on a device it raised this
    # ValueError ("targets 'labels' must be a torch.int64 tensor of shape ...", tests/test_gpu_augment.py).  A malformed call is a ValueError wherever
    # its tensors live, as for the four other consumers
    "padded: a wrong rank": [(V, "targets 'labels' must be torch.int64 with 2 dimensions"), (V, "targets 'ids' must be torch.int64 with 2 dimensions"),
                             (V, "targets 'labels' must be"), (V, "targets 'labels' must be torch.int64 with 2 dimensions"), (V, "'scores' must be torch.float32 with 2 dimensions")],
    "padded: a wrong shape": [(V, "expected target boxes [2,Gmax,4], labels [2,Gmax], count [2], got"), (V, "expected target boxes [2,Gmax,4], ids [2,Gmax], count [2], got"),
                              (V, "count [2], got"), (V, "expected target boxes [2,Gmax,4], labels [2,Gmax], count [2], got"), (V, "count [")],
    "padded: CPU tensors": [(R, "runs on HIP devices only (no CPU fallback)")] * 5,
    "padded: a tuple of CPU tensors": [(R, "HIP devices only"), (R, "HIP devices only"), (R, "HIP devices only"), (R, "HIP devices only"), LIST_FORM],
}


@pytest.mark.parametrize("case", list(EXPECTED))
@pytest.mark.parametrize("consumer", list(SPECS))
def test_reader_refuses_and_reads_with_each_consumers_spec(consumer, case):
    targets, expected = inputs(consumer)[case], EXPECTED[case][list(SPECS).index(consumer)]
    if expected is not None:
        with pytest.raises(expected[0]) as e:
            read(consumer, targets)
        assert type(e.value) is expected[0] and expected[1] in str(e.value) and str(e.value).startswith(consumer)
        return
    t, Gmax = read(consumer, targets)
    n, most = len(targets), max(len(d["boxes"]) for d in targets)
    assert Gmax == max(1, most) and t["boxes"].shape == (n, Gmax, 4) and t["boxes"].dtype == SPECS[consumer][0][0].numpy
    assert t["count"].dtype == np.int32 and t["count"].tolist() == [len(d["boxes"]) for d in targets]
    for name, dtype in named(consumer):
        if name == "ids" and consumer == "augment_batch":
            assert t["ids"] is None
            continue
        assert t[name].shape == (n, Gmax) and t[name].dtype == dtype
        for i, d in enumerate(targets):
            m = len(d["boxes"])
            assert np.array_equal(t[name][i, :m], np.asarray(d[name]).astype(dtype)) and not t[name][i, m:].any()
            assert np.array_equal(t["boxes"][i, :m], np.asarray(d["boxes"], dtype=t["boxes"].dtype).reshape(m, 4)) and not t["boxes"][i, m:].any()


def test_optional_ids_are_read_when_every_image_has_them_and_the_predicate_tells_the_forms_apart():
    t, Gmax = _targets.read_list([image("augment_batch", 2, ids=[7, 8]), image("augment_batch", 0, ids=[])], N, augment._COLUMNS, "augment_batch", optional=("ids",))
    assert Gmax == 2 and t["ids"].tolist() == [[7, 8], [0, 0]] and t["ids"].dtype == np.int64
    three = tuple(torch.zeros(1) for _ in range(3))
    assert _targets.is_padded({}) and _targets.is_padded(three) and _targets.is_padded(list(three)) and not _targets.is_padded(three, (4,))
    assert _targets.is_padded(three + three[:1], (3, 4)) and not _targets.is_padded([{}, {}, {}]) and not _targets.is_padded(three[:2] + (None,))
    assert not _targets.is_padded([]) and not _targets.is_padded(None)
