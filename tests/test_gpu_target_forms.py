"""GPU: the three spellings of the same targets (the list of per-image dicts, the padded device dict, the padded device tuple) give the same
bytes out of each consumer of the shared reader (_targets.py): augment_batch, warp_batch, detection_loss, reid_loss and CocoEvaluator.update.
The smallest inputs that have padding, an empty image and Gmax > 1: two 8 x 8 frames, an 8 x 8 canvas, a 2 x 2 map at stride 4, 2 classes,
4 embedding channels, 3 identities; one image has three boxes, the other none."""
import numpy as np
import pytest
import torch

import centernet_lightning_amd as cl

pytestmark = pytest.mark.gpu

BOXES = np.array([[1.0, 1.0, 4.0, 3.0], [4.0, 2.0, 3.0, 5.0], [0.0, 5.0, 6.0, 2.0]])          # x y w h on the integer grid of the 8 x 8 frame
LABELS, IDS = np.array([1, 0, 1]), np.array([2, 0, 1])


def as_bytes(x):
    """Every tensor of a result, by name or position, as bytes."""
    if isinstance(x, dict):
        return {k: as_bytes(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [as_bytes(v) for v in x]
    return (str(x.dtype), tuple(x.shape), x.detach().cpu().numpy().tobytes()) if isinstance(x, torch.Tensor) else x


def test_list_dict_and_tuple_targets_give_the_same_bytes():
    dev = torch.device("cuda")
    rows = [{"boxes": BOXES, "labels": LABELS, "ids": IDS}, {"boxes": np.zeros((0, 4)), "labels": [], "ids": []}]
    boxes, labels, ids = torch.zeros((2, 3, 4), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64)
    boxes[0], labels[0], ids[0] = torch.from_numpy(BOXES), torch.from_numpy(LABELS), torch.from_numpy(IDS)
    padded = {"boxes": boxes.to(dev), "labels": labels.to(dev), "ids": ids.to(dev), "count": torch.tensor([3, 0], dtype=torch.int32, device=dev)}
    four = (padded["boxes"], padded["labels"], padded["count"], padded["ids"])
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (2, 8, 8, 3), generator=g, dtype=torch.uint8).to(dev)
    heat, box, reid = (torch.randn((2, c, 2, 2), generator=g).to(dev) for c in (2, 4, 4))
    classifier = {k: v.to(dev) for k, v in dict(W1=torch.randn((4, 4), generator=g), gamma=torch.ones(4), beta=torch.zeros(4), running_mean=torch.zeros(4),
                                                running_var=torch.ones(4), W2=torch.randn((3, 4), generator=g), b2=torch.zeros(3)).items()}
    a_plan = cl.sample_augment([(8, 8)] * 2, 8, 8, np.random.default_rng(0), flip=1.0, crop=False)
    w_plan = cl.sample_warp([(8, 8)] * 2, 8, 8, np.random.default_rng(0), rotate=10, crop=False)
    dets = {"bboxes": torch.tensor([[[1, 1, 5, 4], [4, 2, 7, 7], [0, 0, 2, 2]], [[0, 0, 3, 3], [1, 1, 2, 2], [2, 2, 6, 6]]], dtype=torch.float32, device=dev),
            "scores": torch.tensor([[0.9, 0.8, 0.3], [0.5, 0.4, 0.2]], device=dev), "labels": torch.tensor([[1, 0, 1], [0, 1, 1]], device=dev),
            "count": torch.tensor([3, 3], dtype=torch.int32, device=dev)}
    det_rows = [{"boxes": torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], 1).cpu(), "scores": s.cpu(), "labels": lab.cpu()}
                for b, s, lab in zip(dets["bboxes"], dets["scores"], dets["labels"])]

    def coco(preds, targets):
        ev = cl.CocoEvaluator(2)
        ev.update(preds, targets)
        return ev.state(), ev.get_metrics()

    consumers = {          # name: (the call on one spelling of the targets, the spellings it takes)
        "augment_batch": (lambda t: cl.augment_batch(frames, a_plan, t), (rows, padded, four)),
        "warp_batch": (lambda t: cl.warp_batch(frames, w_plan, t), (rows, padded, four)),
        "augment_batch without ids": (lambda t: cl.augment_batch(frames, a_plan, t),
                                      ([{k: v for k, v in d.items() if k != "ids"} for d in rows], {k: v for k, v in padded.items() if k != "ids"}, four[:3])),
        "detection_loss": (lambda t: cl.detection_loss(heat, box, t), (rows, padded, four[:3])),
        "reid_loss": (lambda t: cl.reid_loss(reid, t, classifier, update_stats=False), (rows, padded, four)),
        "CocoEvaluator.update": (lambda t: coco(dets, t), (rows, padded, four[:3])),
        "CocoEvaluator.update, detections": (lambda p: coco(p, rows), (det_rows, dets)),
    }
    for name, (call, spellings) in consumers.items():
        first = as_bytes(call(spellings[0]))
        for other in spellings[1:]:
            assert as_bytes(call(other)) == first, (name, type(other).__name__)
    # and the targets were read, not dropped: three boxes of image 0 reach the outputs
    assert int(cl.augment_batch(frames, a_plan, rows)[1]["count"][0]) == 3 and int(cl.reid_loss(reid, four, classifier, update_stats=False)["num_rows"]) == 3
    assert float(cl.detection_loss(heat, box, four[:3])["per_image"][0, 3]) >= 1.0
