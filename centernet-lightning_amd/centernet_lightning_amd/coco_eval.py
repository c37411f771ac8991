"""COCO box evaluation on the GPU: the reference's CocoEvaluator (eval/coco.py: update / get_metrics / reset, the same twelve metric
names in the same order) without pycocotools, and without the detections leaving the device between gather_detection2d and the numbers.

update() runs ONE launch per batch (cnl_coco_match_f64, csrc/coco_eval.hip: class ranks and the 4 area ranges x 10 thresholds of
matching per image) and appends one record per detection slot to growing device buffers; get_metrics() orders the epoch's records with
two stable device sorts, runs ONE launch (cnl_coco_accumulate_f64) and downloads precision / recall once.  The rule is COCOeval's for
the records the reference builds (no crowds), stated in include/centernet_gfx950.h and restated in numpy in tests/coco_eval_ref.py; the
two agree bit for bit.  No CPU fallback: a missing device or library raises.
"""
import ctypes

import numpy as np
import torch

from . import _gather, _lib

METRIC_NAMES = ("mAP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "mAR", "AR_small", "AR_medium", "AR_large")
MAX_PER_IMAGE = 1024          # detections (k) and ground truths (Gmax) per image: csrc/coco_eval.hip keeps an image in LDS
T, R, A, M = 10, 101, 4, 3    # thresholds, recall points, area ranges, maxDets
_RECORD = (("score", torch.float32), ("label", torch.int64), ("rank", torch.int32), ("matched", torch.int64), ("ignored", torch.int64))


def summarize(precision, recall):
    """precision [T, R, K, A, M] and recall [T, K, A, M] (numpy float64, -1 = no ground truth) -> the twelve numbers, as COCOeval.summarize:
    the mean of the entries > -1 of a slice, -1 for a slice without any."""
    def mean(x):
        x = x[x > -1]
        return float(x.mean()) if x.size else -1.0
    values = (mean(precision[:, :, :, 0, 2]), mean(precision[0, :, :, 0, 2]), mean(precision[5, :, :, 0, 2]), mean(precision[:, :, :, 1, 2]),
              mean(precision[:, :, :, 2, 2]), mean(precision[:, :, :, 3, 2]), mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]),
              mean(recall[:, :, 0, 2]), mean(recall[:, :, 1, 2]), mean(recall[:, :, 2, 2]), mean(recall[:, :, 3, 2]))
    return dict(zip(METRIC_NAMES, values))


def _upload(parts, dev):
    """numpy arrays (int64 / float64 / int32) -> device tensors of the same dtype and shape, through ONE pinned staging buffer and one
    asynchronous copy (call under torch.cuda.device(dev))."""
    words = [-(-p.nbytes // 8) for p in parts]
    buf = np.zeros((max(sum(words), 1),), dtype=np.int64)
    at = 0
    for p, w in zip(parts, words):
        buf[at:at + w].view(np.uint8)[:p.nbytes] = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
        at += w
    dev_buf = _gather.upload(buf, dev)
    out, at = [], 0
    for p, w in zip(parts, words):
        out.append(dev_buf[at:at + w].view(getattr(torch, p.dtype.name))[:p.size].view(p.shape))
        at += w
    return out


def _as_numpy(x, dtype, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    try:
        return np.asarray(x).astype(dtype, copy=False)
    except (TypeError, ValueError) as e:
        raise ValueError(f"CocoEvaluator.update: {what} is not numeric: {e}") from e


def _per_image(items, what, with_scores):
    """The reference's per-image dicts -> [(boxes [n, 4] xywh, labels [n] int64[, scores [n] float32])] as numpy."""
    out = []
    for i, d in enumerate(items):
        if not isinstance(d, dict) or "boxes" not in d or "labels" not in d or (with_scores and "scores" not in d):
            raise ValueError(f"CocoEvaluator.update: {what}[{i}] must be a dict with 'boxes', 'labels'" + (", 'scores'" if with_scores else ""))
        boxes = _as_numpy(d["boxes"], np.float32 if with_scores else np.float64, f"{what}[{i}]['boxes']")
        if boxes.size == 0:
            boxes = boxes.reshape(0, 4)
        labels = _as_numpy(d["labels"], np.int64, f"{what}[{i}]['labels']").reshape(-1)
        if boxes.ndim != 2 or boxes.shape[1] != 4 or boxes.shape[0] != labels.shape[0]:
            raise ValueError(f"CocoEvaluator.update: {what}[{i}] has boxes {boxes.shape} and labels {labels.shape}; expected [n, 4] and [n]")
        rec = (boxes, labels)
        if with_scores:
            scores = _as_numpy(d["scores"], np.float32, f"{what}[{i}]['scores']").reshape(-1)
            if scores.shape[0] != labels.shape[0]:
                raise ValueError(f"CocoEvaluator.update: {what}[{i}] has {scores.shape[0]} scores for {labels.shape[0]} labels")
            rec += (scores,)
        if labels.shape[0] > MAX_PER_IMAGE:
            raise ValueError(f"CocoEvaluator.update: {what}[{i}] has {labels.shape[0]} boxes; at most {MAX_PER_IMAGE} per image are supported")
        out.append(rec)
    return out


def _check_tensors(named, what):
    """[(name, tensor, dtype, dimensions)]: a malformed call is a ValueError wherever its tensors live, so this runs before _one_device."""
    for name, t, dtype, dims in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"CocoEvaluator.update: {what} '{name}' must be a tensor, got {type(t).__name__}")
        if t.dtype != dtype or t.dim() != dims:
            raise ValueError(f"CocoEvaluator.update: {what} '{name}' must be {dtype} with {dims} dimensions, got {t.dtype} {tuple(t.shape)}")


def _one_device(named, what):
    """All on one HIP device (RuntimeError for a CPU tensor: no CPU fallback) -> that device."""
    _gather.require_hip([t for (_, t, _, _) in named], "CocoEvaluator.update")
    dev = named[0][1].device
    for name, t, _, _ in named:
        if t.device != dev:
            raise ValueError(f"CocoEvaluator.update: {what} tensors live on different devices ({dev}, {t.device})")
    return dev


class CocoEvaluator:
    """CocoEvaluator(num_classes, device=None) — drop-in for the reference's (eval/coco.py:21).  `device`: the HIP device of the state;
    None takes the device of the first update."""
    metric_names = METRIC_NAMES

    def __init__(self, num_classes, device=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= 1 << 20:
            raise ValueError(f"CocoEvaluator: num_classes must be an int in 1..2^20, got {num_classes!r}")
        self.num_classes = num_classes
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("CocoEvaluator runs on HIP devices only (no CPU fallback)")
        self._buf = None
        self._npig = None
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """Forget every record (the device buffers are kept for the next epoch)."""
        self._n = 0                  # records: one per detection slot seen
        self.num_images = 0
        self.precision = None        # numpy [10, 101, K, 4, 3] / [10, K, 4, 3] after get_metrics
        self.recall = None
        if self._npig is not None:
            self._npig.zero_()

    def _bind(self, dev):
        if self.device is None or self.device.index is None:       # ("cuda" without an ordinal: the first input decides)
            self.device = dev
        elif dev != self.device:
            raise ValueError(f"CocoEvaluator: state on {self.device}, input on {dev}")
        if self._npig is None:
            self._npig = torch.zeros((self.num_classes, A), dtype=torch.int64, device=self.device)

    def _reserve(self, extra):
        """Room for `extra` more records: the buffers double, so an epoch of equal batches reallocates O(log) times, not once per batch."""
        need = self._n + extra
        cap = 0 if self._buf is None else self._buf["score"].shape[0]
        if need <= cap:
            return
        cap = max(need, 2 * cap, 4096)
        new = {name: torch.empty((cap,), dtype=dtype, device=self.device) for name, dtype in _RECORD}
        if self._buf is not None and self._n:
            for name, _ in _RECORD:
                new[name][:self._n].copy_(self._buf[name][:self._n])
        self._buf = new

    def state(self):
        """The records so far — {"num_classes", "num_images", "score", "label", "rank", "matched", "ignored" (one entry per detection
        slot, in order of arrival), "npig" [K, 4]} as device tensors (copies).  A record depends on its own image only, so another
        evaluator that merge()s this state after its own records equals one evaluator that saw both shards in that order."""
        if self.device is None:
            raise RuntimeError("CocoEvaluator.state: nothing has been evaluated yet")
        with torch.cuda.device(self.device):
            self._reserve(0)
            out = {name: (self._buf[name][:self._n].clone() if self._buf is not None else torch.empty((0,), dtype=dtype, device=self.device))
                   for name, dtype in _RECORD}
            out["npig"] = self._npig.clone()
        out["num_classes"], out["num_images"] = self.num_classes, self.num_images
        return out

    def merge(self, state):
        """Append another evaluator's state() after this one's records (how shards and ranks combine; no collective is involved)."""
        if not isinstance(state, dict) or any(name not in state for name in ("npig", "num_classes", "num_images") + tuple(n for n, _ in _RECORD)):
            raise ValueError("CocoEvaluator.merge expects the dict another evaluator's state() returned")
        if state["num_classes"] != self.num_classes:
            raise ValueError(f"CocoEvaluator.merge: state of {state['num_classes']} classes into an evaluator of {self.num_classes}")
        n = int(state["score"].shape[0])
        for name, dtype in _RECORD:
            t = state[name]
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,):
                raise ValueError(f"CocoEvaluator.merge: '{name}' must be {dtype} [{n}]")
        if not isinstance(state["npig"], torch.Tensor) or state["npig"].dtype != torch.int64 or tuple(state["npig"].shape) != (self.num_classes, A):
            raise ValueError(f"CocoEvaluator.merge: 'npig' must be int64 [{self.num_classes}, {A}]")
        _gather.require_hip([state["npig"]] + [state[name] for name, _ in _RECORD], "CocoEvaluator.merge")
        self._bind(self.device if self.device is not None else state["npig"].device)
        with torch.cuda.device(self.device):
            self._reserve(n)
            for name, _ in _RECORD:
                self._buf[name][self._n:self._n + n].copy_(state[name])
            self._npig += state["npig"].to(self.device)
        self._n += n
        self.num_images += int(state["num_images"])

    # ------------------------------------------------------------------ update
    def _detections(self, preds):
        """-> (boxes [N,k,4] f32 xyxy, scores, labels, count or None, N, k) as device tensors, or as numpy for the list form."""
        if isinstance(preds, dict):
            boxes = preds.get("bboxes", preds.get("boxes"))
            if boxes is None or "scores" not in preds or "labels" not in preds:
                raise ValueError("CocoEvaluator.update: the detections need 'bboxes' (or 'boxes'), 'scores' and 'labels'")
            named = [("bboxes", boxes, torch.float32, 3), ("scores", preds["scores"], torch.float32, 2), ("labels", preds["labels"], torch.int64, 2)]
            count = preds.get("count")
            if count is not None:
                if not isinstance(count, torch.Tensor) or count.dtype not in (torch.int32, torch.int64) or count.dim() != 1:
                    raise ValueError("CocoEvaluator.update: 'count' must be an int32 / int64 [N] tensor")
                named.append(("count", count, count.dtype, 1))
            _check_tensors(named, "detections")
            N, k = int(boxes.shape[0]), int(boxes.shape[1])
            if boxes.shape[2] != 4 or tuple(preds["scores"].shape) != (N, k) or tuple(preds["labels"].shape) != (N, k) or \
                    (count is not None and count.shape[0] != N):
                raise ValueError(f"CocoEvaluator.update: expected bboxes [N,k,4], scores [N,k], labels [N,k] (count [N]), got {tuple(boxes.shape)}, "
                                 f"{tuple(preds['scores'].shape)}, {tuple(preds['labels'].shape)}" + (f", {tuple(count.shape)}" if count is not None else ""))
            if not 1 <= k <= MAX_PER_IMAGE:
                raise ValueError(f"CocoEvaluator.update: k = {k} detections per image; 1..{MAX_PER_IMAGE} are supported")
            dev = _one_device(named, "detections")
            if count is not None and count.dtype != torch.int32:
                count = count.to(torch.int32)
            return dev, (boxes.contiguous(), preds["scores"].contiguous(), preds["labels"].contiguous(),
                         None if count is None else count.contiguous()), N, k
        if not isinstance(preds, (list, tuple)):
            raise ValueError(f"CocoEvaluator.update: detections must be the device dict of gather_detection2d or a list of per-image dicts, "
                             f"got {type(preds).__name__}")
        images = _per_image(preds, "preds", True)
        N, k = len(images), max([1] + [len(lab) for (_, lab, _) in images])
        boxes, scores = np.zeros((N, k, 4), dtype=np.float32), np.zeros((N, k), dtype=np.float32)
        labels, count = np.zeros((N, k), dtype=np.int64), np.zeros((N,), dtype=np.int32)
        for i, (b, lab, s) in enumerate(images):
            n = len(lab)
            boxes[i, :n, :2] = b[:, :2]
            boxes[i, :n, 2:] = b[:, :2] + b[:, 2:]       # fp32: the kernel's w = x2 - x1 gives w back only when x + w is exact
            scores[i, :n], labels[i, :n], count[i] = s, lab, n
        return None, (boxes, scores, labels, count), N, k

    def _targets(self, targets, N):
        """-> (device or None, (boxes [N,Gmax,4] f64 xywh, labels [N,Gmax] i64, count [N] i32), Gmax)"""
        if isinstance(targets, dict) or (isinstance(targets, (list, tuple)) and len(targets) == 3 and all(isinstance(t, torch.Tensor) for t in targets)):
            if isinstance(targets, dict):
                if any(name not in targets for name in ("boxes", "labels", "count")):
                    raise ValueError("CocoEvaluator.update: device targets need 'boxes' [N,Gmax,4] f64, 'labels' [N,Gmax] i64 and 'count' [N] i32")
                targets = (targets["boxes"], targets["labels"], targets["count"])
            boxes, labels, count = targets
            named = [("boxes", boxes, torch.float64, 3), ("labels", labels, torch.int64, 2), ("count", count, torch.int32, 1)]
            _check_tensors(named, "targets")
            Gmax = int(boxes.shape[1])
            if tuple(boxes.shape) != (N, Gmax, 4) or tuple(labels.shape) != (N, Gmax) or tuple(count.shape) != (N,):
                raise ValueError(f"CocoEvaluator.update: expected target boxes [{N},Gmax,4], labels [{N},Gmax], count [{N}], got "
                                 f"{tuple(boxes.shape)}, {tuple(labels.shape)}, {tuple(count.shape)}")
            if not 1 <= Gmax <= MAX_PER_IMAGE:
                raise ValueError(f"CocoEvaluator.update: Gmax = {Gmax} ground truths per image; 1..{MAX_PER_IMAGE} are supported")
            dev = _one_device(named, "targets")
            return dev, (boxes.contiguous(), labels.contiguous(), count.contiguous()), Gmax
        if not isinstance(targets, (list, tuple)):
            raise ValueError(f"CocoEvaluator.update: targets must be a list of per-image dicts or padded device tensors, got {type(targets).__name__}")
        if len(targets) != N:
            raise ValueError(f"CocoEvaluator.update: {N} images of detections against {len(targets)} of targets")
        images = _per_image(targets, "targets", False)
        Gmax = max([1] + [len(lab) for (_, lab) in images])
        boxes, labels, count = np.zeros((N, Gmax, 4), dtype=np.float64), np.zeros((N, Gmax), dtype=np.int64), np.zeros((N,), dtype=np.int32)
        for i, (b, lab) in enumerate(images):
            boxes[i, :len(lab)], labels[i, :len(lab)], count[i] = b, lab, len(lab)
        return None, (boxes, labels, count), Gmax

    def update(self, preds, targets):
        """One batch.  preds: the device dict of gather_detection2d / detect_frames / detect_tiled as it is — "bboxes" (or "boxes")
        [N,k,4] fp32 x1 y1 x2 y2, "scores" [N,k], "labels" [N,k] int64 and optionally "count" [N] (the slots that hold detections);
        k <= 1024.  For drop-in use also the reference's form, a list of per-image dicts {"boxes" [n,4] x y w h, "scores", "labels"}
        (numpy or CPU tensors): the corners x + w, y + h are rebuilt in fp32 for the kernel, which is exact only when those sums are
        exact in fp32 (integer-grid boxes, say) — the device form is the one to use.
        targets: the reference's list of per-image {"boxes" [g,4] x y w h, "labels" [g]} (at most 1024 per image; padded and uploaded
        once through a pinned buffer), or padded device tensors (boxes [N,Gmax,4] float64, labels [N,Gmax] int64, count [N] int32) as a
        tuple or a dict with those keys.  One launch, no device sync."""
        d_dev, dets, N, k = self._detections(preds)
        g_dev, gts, Gmax = self._targets(targets, N)
        dev = d_dev if d_dev is not None else g_dev if g_dev is not None else self.device
        if dev is None or dev.index is None:                # nothing came from a device: the evaluator's own, or the current one
            if not torch.cuda.is_available():
                raise RuntimeError("CocoEvaluator runs on HIP devices only (no CPU fallback)")
            dev = torch.device("cuda", torch.cuda.current_device())
        if d_dev is not None and g_dev is not None and d_dev != g_dev:
            raise ValueError(f"CocoEvaluator.update: detections on {d_dev}, targets on {g_dev}")
        self._bind(dev)
        if N == 0:
            return
        lib = _lib.load()
        with torch.cuda.device(self.device):
            host = (list(dets) if d_dev is None else []) + (list(gts) if g_dev is None else [])
            if host:                                        # everything that came as numpy goes up in one copy
                up = _upload(host, self.device)
                if d_dev is None:
                    dets, up = up[:4], up[4:]
                if g_dev is None:
                    gts = up
            boxes, scores, labels, count = dets
            self._reserve(N * k)
            at, buf = self._n, self._buf
            buf["score"][at:at + N * k].copy_(scores.reshape(-1))
            buf["label"][at:at + N * k].copy_(labels.reshape(-1))
            _lib.check(lib.cnl_coco_match_f64(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), None if count is None else count.data_ptr(),
                                              gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), N, k, Gmax, self.num_classes,
                                              buf["rank"].data_ptr() + 4 * at, buf["matched"].data_ptr() + 8 * at, buf["ignored"].data_ptr() + 8 * at,
                                              self._npig.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                       "cnl_coco_match_f64")
        self._n += N * k
        self.num_images += N

    # ------------------------------------------------------------------ metrics
    def get_metrics(self):
        """-> {metric name: float} for the twelve names of `metric_names`, in that order; .precision [10,101,K,4,3] and .recall
        [10,K,4,3] (numpy float64, -1 where a category has no ground truth in a range) are kept.  Two stable device sorts (descending
        score, then category), one launch, ONE download; the -1-aware means are host numpy."""
        if self.device is None:
            raise RuntimeError("CocoEvaluator.get_metrics: nothing has been evaluated yet")
        K, n, dev = self.num_classes, self._n, self.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            self._reserve(0)
            buf = self._buf if self._buf is not None else {name: torch.empty((0,), dtype=dtype, device=dev) for name, dtype in _RECORD}
            rank = buf["rank"][:n]
            by_score = torch.sort(buf["score"][:n] + 0.0, descending=True, stable=True).indices         # (+ 0: -0 and +0 are one score)
            category = torch.where(rank >= 0, buf["label"][:n], K)[by_score]                              # dropped records behind the last category
            category, by_category = torch.sort(category, stable=True)
            order = by_score[by_category]
            first = torch.searchsorted(category, torch.arange(K + 1, device=dev, dtype=torch.int64)).contiguous()
            rank, matched, ignored = rank[order].contiguous(), buf["matched"][:n][order].contiguous(), buf["ignored"][:n][order].contiguous()
            out = torch.empty((T * R * K * A * M + T * K * A * M,), dtype=torch.float64, device=dev)
            n_pr = T * R * K * A * M
            _lib.check(lib.cnl_coco_accumulate_f64(rank.data_ptr(), matched.data_ptr(), ignored.data_ptr(), first.data_ptr(), self._npig.data_ptr(),
                                                   n, K, out.data_ptr(), out.data_ptr() + 8 * n_pr,
                                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "cnl_coco_accumulate_f64")
            host = out.cpu().numpy()
        self.precision = host[:n_pr].reshape(T, R, K, A, M)
        self.recall = host[n_pr:].reshape(T, K, A, M)
        return summarize(self.precision, self.recall)
