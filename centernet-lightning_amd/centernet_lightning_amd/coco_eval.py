"""COCO box evaluation on the GPU: the reference's CocoEvaluator (eval/coco.py: update / get_metrics / reset, the same twelve metric
names in the same order) without pycocotools, and without the detections leaving the device between gather_detection2d and the numbers.

update() runs ONE launch per batch (cnl_coco_match_f64, csrc/coco_eval.hip: class ranks and the 4 area ranges x 10 thresholds of
matching per image) and appends one record per detection slot to growing device buffers; get_metrics() orders the epoch's records with
two stable device sorts, runs ONE launch (cnl_coco_accumulate_f64) and downloads precision / recall once.  The rule is COCOeval's for
the records the reference builds (no crowds), stated in include/centernet_gfx950.h and restated in numpy in tests/coco_eval_ref.py; the
two agree bit for bit.  No CPU fallback: a missing device or library raises.
"""
import torch

from . import _gather, _lib
from . import _targets as _t

METRIC_NAMES = ("mAP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "mAR", "AR_small", "AR_medium", "AR_large")
MAX_PER_IMAGE = 1024          # detections (k) and ground truths (Gmax) per image: csrc/coco_eval.hip keeps an image in LDS
T, R, A, M = 10, 101, 4, 3    # thresholds, recall points, area ranges, maxDets
_DETECTIONS = _t.columns(("scores", "float32"), ("labels", "int64"), boxes="float32")       # the predictions, in either form
_DETECTIONS_COUNT64 = _DETECTIONS[:-1] + (_DETECTIONS[-1]._replace(torch=torch.int64),)        # gather_detection2d's count may be int64
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
        """-> (device or None, (boxes [N,k,4] f32 xyxy, scores, labels, count or None) as device tensors, or as numpy for the list form, N, k)"""
        what = "CocoEvaluator.update"
        if isinstance(preds, dict):
            boxes, count = preds.get("bboxes", preds.get("boxes")), preds.get("count")
            if boxes is None or "scores" not in preds or "labels" not in preds:
                raise ValueError(f"{what}: the detections need 'bboxes' (or 'boxes'), 'scores' and 'labels'")
            if count is not None and (not isinstance(count, torch.Tensor) or count.dtype not in (torch.int32, torch.int64) or count.dim() != 1):
                raise ValueError(f"{what}: 'count' must be an int32 / int64 [N] tensor")
            narrow = count is not None and count.dtype != torch.int32          # an int64 count is read as it is and made int32 once all is checked
            spec = _DETECTIONS_COUNT64 if narrow else _DETECTIONS
            t, k, dev = _t.read_padded({"boxes": boxes, "scores": preds["scores"], "labels": preds["labels"], "count": count}, None, spec, what,
                                       arg="detections", one="detection", dim="k", optional=("count",), cap=MAX_PER_IMAGE)
            return dev, (t["boxes"], t["scores"], t["labels"], t["count"].to(torch.int32) if narrow else t["count"]), int(boxes.shape[0]), k
        if not isinstance(preds, (list, tuple)):
            raise ValueError(f"{what}: detections must be the device dict of gather_detection2d or a list of per-image dicts, got {type(preds).__name__}")
        t, k = _t.read_list(preds, None, _DETECTIONS, what, arg="preds", cap=MAX_PER_IMAGE)
        t["boxes"][..., 2:] += t["boxes"][..., :2]       # x y w h -> corners in fp32: the kernel's w = x2 - x1 gives w back only when x + w is exact
        return None, (t["boxes"], t["scores"], t["labels"], t["count"]), len(preds), k

    def _targets(self, targets, N):
        """-> (device or None, (boxes [N,Gmax,4] f64 xywh, labels [N,Gmax] i64, count [N] i32), Gmax)"""
        what = "CocoEvaluator.update"
        if _t.is_padded(targets):
            t, Gmax, dev = _t.read_padded(targets, N, _t.LABELS, what, cap=MAX_PER_IMAGE)
        else:
            (t, Gmax), dev = _t.read_list(targets, N, _t.LABELS, what, against="detections", cap=MAX_PER_IMAGE), None
        return dev, (t["boxes"], t["labels"], t["count"]), Gmax

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
                up = _gather.upload_parts(host, self.device)
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
                                              self._npig.data_ptr(), _lib.stream(self.device)),
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
                                                   _lib.stream(dev)), "cnl_coco_accumulate_f64")
            host = out.cpu().numpy()
        self.precision = host[:n_pr].reshape(T, R, K, A, M)
        self.recall = host[n_pr:].reshape(T, K, A, M)
        return summarize(self.precision, self.recall)
