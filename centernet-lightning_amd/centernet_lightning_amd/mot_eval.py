"""MOT evaluation on the GPU: the reference's evaluate_mot_tracking_sequence (eval/mot_challenge.py -> TrackEval's HOTA, CLEAR and
Identity for MotChallenge2DBox) without TrackEval, without the folder of text files, and for any number of sequences at once.

update() only collects frames on the host.  get_metrics() relabels the ids of every sequence to 0..n-1 (ascending original id, as
TrackEval's preprocessing does), pools all sequences into one set of arrays, uploads them in ONE copy, runs the launches of
csrc/mot_eval.hip (similarity, HOTA, CLEAR, Identity: every sequence goes through the same launches) and downloads the per-sequence
sums in ONE copy; the final fields and COMBINED_SEQ are host arithmetic on those.  The rule is stated in include/centernet_gfx950.h and
restated in numpy + scipy in tests/mot_eval_ref.py; the two agree bit for bit.  No CPU fallback: a missing device or library raises.
The one host solve is Identity's single assignment for a sequence with more than 1024 ground-truth + tracker ids, which the solver's
LDS does not hold: its counts come back from the device and scipy solves that one problem.
"""
import ctypes

import numpy as np
import torch

from . import _gather, _lib

ALPHA = np.arange(0.05, 0.99, 0.05)        # TrackEval's HOTA.array_labels: 19 float64 values
MAX_SHORT, MAX_LONG = 1024, 4096           # objects of a frame on its smaller / larger side (the solver's LDS)
MAX_IDENTITY = 1024                        # ground-truth + tracker ids of a sequence whose Identity assignment runs on the device
HOTA_ARRAYS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA", "OWTA", "HOTA_TP", "HOTA_FN", "HOTA_FP")
CLEAR_FIELDS = ("MOTA", "MOTP", "MODA", "CLR_Re", "CLR_Pr", "MTR", "PTR", "MLR", "sMOTA", "CLR_F1", "FP_per_frame", "MOTAL", "MOTP_sum",
                "CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "CLR_Frames")
IDENTITY_FIELDS = ("IDF1", "IDR", "IDP", "IDTP", "IDFN", "IDFP")
_CLEAR_INT = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag")
_STATUS = {1: "a score that is not finite", 2: "an infeasible assignment", 3: "a problem larger than the solver's limits", 5: "inconsistent tables"}


# ---------------------------------------------------------------------------------------------------------------- host fields
def hota_final(res):
    """LocA_sum / AssA / AssRe / AssPr / HOTA_TP / HOTA_FN / HOTA_FP (19-vectors) -> every HOTA field, as TrackEval's _compute_final_fields."""
    tp, fn, fp = (res[k].astype(np.float64) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP"))
    out = dict(res)
    if "LocA" not in out:
        out["LocA"] = np.maximum(1e-10, res["LocA_sum"]) / np.maximum(1e-10, tp)
    out["DetRe"] = tp / np.maximum(1.0, tp + fn)
    out["DetPr"] = tp / np.maximum(1.0, tp + fp)
    out["DetA"] = tp / np.maximum(1.0, tp + fn + fp)
    out["HOTA"] = np.sqrt(out["DetA"] * out["AssA"])
    out["OWTA"] = np.sqrt(out["DetRe"] * out["AssA"])
    return out


def clear_final(res):
    """The CLEAR sums -> the final fields (TrackEval's CLEAR._compute_final_fields)."""
    out = dict(res)
    tp, fn, fp, idsw = (float(res[k]) for k in ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW"))
    ids = float(res["MT"] + res["ML"] + res["PT"])
    out["MTR"], out["MLR"], out["PTR"] = (float(res[k] / np.maximum(1.0, ids)) for k in ("MT", "ML", "PT"))
    out["CLR_Re"] = float(tp / np.maximum(1.0, tp + fn))
    out["CLR_Pr"] = float(tp / np.maximum(1.0, tp + fp))
    out["MODA"] = float((tp - fp) / np.maximum(1.0, tp + fn))
    out["MOTA"] = float((tp - fp - idsw) / np.maximum(1.0, tp + fn))
    out["MOTP"] = float(res["MOTP_sum"] / np.maximum(1.0, tp))
    out["sMOTA"] = float((res["MOTP_sum"] - fp - idsw) / np.maximum(1.0, tp + fn))
    out["CLR_F1"] = float(tp / np.maximum(1.0, tp + 0.5 * fn + 0.5 * fp))
    out["FP_per_frame"] = float(fp / np.maximum(1.0, float(res["CLR_Frames"])))
    safe_log_idsw = float(np.log10(idsw)) if idsw > 0 else idsw
    out["MOTAL"] = float((tp - fp - safe_log_idsw) / np.maximum(1.0, tp + fn))
    return out


def identity_final(res):
    out = dict(res)
    tp, fn, fp = (float(res[k]) for k in ("IDTP", "IDFN", "IDFP"))
    out["IDR"] = float(tp / np.maximum(1.0, tp + fn))
    out["IDP"] = float(tp / np.maximum(1.0, tp + fp))
    out["IDF1"] = float(tp / np.maximum(1.0, tp + 0.5 * fp + 0.5 * fn))
    return out


def combine_sequences(per_sequence):
    """{sequence: metrics} in order of arrival -> COMBINED_SEQ, TrackEval's combine_sequences for the three families."""
    seqs = list(per_sequence.values())
    res = {k: sum(m[k] for m in seqs) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP")}
    for k in ("AssRe", "AssPr", "AssA"):
        res[k] = sum(m[k] * m["HOTA_TP"] for m in seqs) / np.maximum(1.0, res["HOTA_TP"])
    res["LocA"] = np.maximum(1e-10, sum(m["LocA"] * m["HOTA_TP"] for m in seqs)) / np.maximum(1e-10, res["HOTA_TP"])
    out = hota_final(res)
    clear = {k: sum(m[k] for m in seqs) for k in _CLEAR_INT + ("CLR_Frames", "MOTP_sum")}
    out.update(clear_final(clear))
    out.update(identity_final({k: sum(m[k] for m in seqs) for k in ("IDTP", "IDFN", "IDFP")}))
    out["summary"] = _summary(out)
    return out


def _summary(m):
    """The HOTA family as TrackEval's tables report it: the mean over alpha of every array field."""
    return {k: float(np.mean(m[k])) for k in HOTA_ARRAYS}


# ---------------------------------------------------------------------------------------------------------------- input
def _boxes(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    try:
        b = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"MotEvaluator.update: {what} is not numeric: {e}") from e
    if b.size == 0:
        b = b.reshape(0, 4)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"MotEvaluator.update: {what} must be [n, 4] x y w h, got {b.shape}")
    if not np.isfinite(b).all():
        raise ValueError(f"MotEvaluator.update: {what} holds a coordinate that is not finite")
    return np.ascontiguousarray(b)


def _ids(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        if not (np.issubdtype(a.dtype, np.floating) and np.isfinite(a).all() and (a == np.floor(a)).all()):
            raise ValueError(f"MotEvaluator.update: {what} must be whole numbers")
    a = a.astype(np.int64).reshape(-1)
    if np.unique(a).size != a.size:
        raise ValueError(f"MotEvaluator.update: {what} repeats an id inside one frame")
    return a


def _relabel(id_frames):
    """Per-frame id arrays of one sequence -> (relabelled ids of all frames, concatenated, int32; the number of ids; frames per id)."""
    flat = np.concatenate(id_frames) if id_frames else np.zeros((0,), np.int64)
    unique, inverse, counts = np.unique(flat, return_inverse=True, return_counts=True)
    return inverse.astype(np.int32).reshape(-1), int(unique.size), counts.astype(np.int32)


def pool(sequences):
    """[(name, frames)] with frames = [(gt boxes, gt ids, pred boxes, pred ids)] -> the pooled host arrays and scalars of cnl_mot_tables
    (numpy; ids relabelled per sequence) plus per-sequence facts the host fields need."""
    gt_boxes, pr_boxes, gt_ids, pr_ids, gt_n, pr_n, frm_seq, gt_count, pr_count = [], [], [], [], [], [], [], [], []
    seq_frm, seq_gid, seq_tid, seq_pair, seq_idm, facts = [0], [0], [0], [0], [0], []
    for s, (name, frames) in enumerate(sequences):
        g_ids, G, g_cnt = _relabel([f[1] for f in frames])
        p_ids, T, p_cnt = _relabel([f[3] for f in frames])
        gt_ids.append(g_ids); pr_ids.append(p_ids); gt_count.append(g_cnt); pr_count.append(p_cnt)
        for f in frames:
            gt_boxes.append(f[0]); pr_boxes.append(f[2]); gt_n.append(len(f[1])); pr_n.append(len(f[3])); frm_seq.append(s)
        seq_frm.append(seq_frm[-1] + len(frames)); seq_gid.append(seq_gid[-1] + G); seq_tid.append(seq_tid[-1] + T)
        seq_pair.append(seq_pair[-1] + G * T)
        seq_idm.append(seq_idm[-1] + ((G + T) ** 2 if G + T <= MAX_IDENTITY else 0))
        facts.append({"name": name, "frames": len(frames), "G": G, "T": T, "n_gt": int(g_ids.size), "n_pr": int(p_ids.size)})
    gt_n, pr_n = np.asarray(gt_n, np.int64), np.asarray(pr_n, np.int64)
    cat = lambda parts, dtype, shape: np.concatenate(parts).astype(dtype, copy=False) if parts else np.zeros(shape, dtype)
    arrays = {"gt_boxes": cat(gt_boxes, np.float64, (0, 4)).reshape(-1, 4), "pr_boxes": cat(pr_boxes, np.float64, (0, 4)).reshape(-1, 4),
              "gt_ids": cat(gt_ids, np.int32, (0,)), "pr_ids": cat(pr_ids, np.int32, (0,)),
              "gt_off": np.concatenate([[0], np.cumsum(gt_n)]).astype(np.int64), "pr_off": np.concatenate([[0], np.cumsum(pr_n)]).astype(np.int64),
              "sim_off": np.concatenate([[0], np.cumsum(gt_n * pr_n)]).astype(np.int64), "frm_seq": np.asarray(frm_seq, np.int32),
              "seq_frm": np.asarray(seq_frm, np.int64), "seq_gid": np.asarray(seq_gid, np.int64), "seq_tid": np.asarray(seq_tid, np.int64),
              "seq_pair": np.asarray(seq_pair, np.int64), "seq_idm": np.asarray(seq_idm, np.int64),
              "gt_count": cat(gt_count, np.int32, (0,)), "pr_count": cat(pr_count, np.int32, (0,))}
    scalars = {"F": len(frm_seq), "S": len(sequences), "n_gt": int(gt_n.sum()), "n_pr": int(pr_n.sum()), "sim_total": int((gt_n * pr_n).sum()),
               "pair_total": seq_pair[-1], "sum_g": seq_gid[-1], "sum_t": seq_tid[-1], "id_total": seq_idm[-1],
               "max_gids": max([f["G"] for f in facts] + [0]), "max_gt_frame": int(gt_n.max(initial=0)), "max_pr_frame": int(pr_n.max(initial=0)),
               "max_frame_pairs": int((gt_n * pr_n).max(initial=0))}
    lo, hi = np.minimum(gt_n, pr_n), np.maximum(gt_n, pr_n)
    if (lo > MAX_SHORT).any() or (hi > MAX_LONG).any():
        raise ValueError(f"MotEvaluator: a frame holds {int(gt_n[np.argmax(hi)])} ground truths and {int(pr_n[np.argmax(hi)])} predictions; at most "
                         f"{MAX_SHORT} on the smaller side and {MAX_LONG} on the larger are supported")
    return arrays, scalars, facts


class _Plain:
    """`nbytes` of device memory for an output or a workspace (tests put guarded allocations in its place)."""
    def __init__(self, nbytes, align, device, name):
        self.nbytes = int(nbytes)
        self.alloc = torch.empty((max(self.nbytes, 8) + 7) // 8, dtype=torch.int64, device=device).view(torch.uint8)
        self.ptr = self.alloc.data_ptr()

    def typed(self, dtype, shape):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return self.alloc[:n].view(dtype).view(shape)


def run(arrays, scalars, device, alloc=_Plain):
    """The launches of one evaluation -> the downloaded sums {"hota_f64" [S,4,19], "hota_i64" [S,3,19], "clear_f64" [S], "clear_i64" [S,8],
    "identity_i64" [S,2], "status" [3,S]} as numpy, and the device tensor of pm.  One upload, one download."""
    lib = _lib.load()
    S = scalars["S"]
    names = list(_lib.MotTables.POINTERS)
    with torch.cuda.device(device):
        stream = _lib.stream(device)
        up = dict(zip(names + ["alpha"], _gather.upload_parts([arrays[n] for n in names] + [ALPHA], device)))
        tab = _lib.MotTables(**{n: up[n].data_ptr() for n in names}, **scalars)
        ref = ctypes.byref(tab)
        sim = alloc(8 * scalars["sim_total"], 8, device, "sim")
        _lib.check(lib.cnl_mot_similarity_f64(ref, sim.ptr, stream), "cnl_mot_similarity_f64")
        outs = {"hota_f64": (torch.float64, (S, 4, 19)), "hota_i64": (torch.int64, (S, 3, 19)), "clear_f64": (torch.float64, (S,)),
                "clear_i64": (torch.int64, (S, 8)), "identity_i64": (torch.int64, (S, 2)), "status_hota": (torch.int32, (S,)),
                "status_clear": (torch.int32, (S,)), "status_identity": (torch.int32, (S,))}
        buf = {n: alloc(int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size(), 8 if dt != torch.int32 else 4, device, n)
               for n, (dt, shape) in outs.items()}
        pm = alloc(4 * scalars["pair_total"], 4, device, "pm")
        ws_bytes = {k: int(getattr(lib, f"cnl_mot_{k}_workspace_bytes")(ref)) for k in ("hota", "clear", "identity")}
        ws = {k: alloc(v, 8, device, f"{k} workspace") for k, v in ws_bytes.items()}
        _lib.check(lib.cnl_mot_hota_f64(ref, sim.ptr, up["alpha"].data_ptr(), buf["hota_f64"].ptr, buf["hota_i64"].ptr, buf["status_hota"].ptr,
                                        ws["hota"].ptr, ws_bytes["hota"], stream), "cnl_mot_hota_f64")
        _lib.check(lib.cnl_mot_clear_f64(ref, sim.ptr, buf["clear_f64"].ptr, buf["clear_i64"].ptr, buf["status_clear"].ptr, ws["clear"].ptr,
                                         ws_bytes["clear"], stream), "cnl_mot_clear_f64")
        _lib.check(lib.cnl_mot_identity_f64(ref, sim.ptr, pm.ptr, buf["identity_i64"].ptr, buf["status_identity"].ptr, ws["identity"].ptr,
                                            ws_bytes["identity"], stream), "cnl_mot_identity_f64")
        parts = [buf[n].typed(dt, shape).reshape(-1).view(torch.uint8) for n, (dt, shape) in outs.items()]
        host = torch.cat(parts).cpu().numpy()                      # the one download (and the one synchronisation)
    got, at = {}, 0
    for n, (dt, shape) in outs.items():
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
        got[n] = host[at:at + nbytes].view(getattr(np, str(dt).split(".")[1])).reshape(shape).copy()
        at += nbytes
    return got, pm, {"sim": sim, "pm": pm, "ws": ws, "ws_bytes": ws_bytes, "out": buf}


def _identity_on_host(pm, g_cnt, p_cnt):
    """Identity's one assignment for a sequence the solver's LDS does not hold: the rule of the header on downloaded counts."""
    from scipy.optimize import linear_sum_assignment
    G, T = len(g_cnt), len(p_cnt)
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fp[G:, :T] = 1e10
    fn[:G, T:] = 1e10
    fn[:G, :T] = g_cnt[:, None]
    fn[np.arange(G), T + np.arange(G)] = g_cnt
    fp[:G, :T] = p_cnt[None, :]
    fp[G + np.arange(T), np.arange(T)] = p_cnt
    fn[:G, :T] -= pm
    fp[:G, :T] -= pm
    rows, cols = linear_sum_assignment(fn + fp)
    return int(fn[rows, cols].sum()), int(fp[rows, cols].sum())


def assemble(got, arrays, scalars, facts, pm):
    """The downloaded sums -> {sequence: every field} + COMBINED_SEQ."""
    for family in ("hota", "clear", "identity"):
        for s, st in enumerate(got[f"status_{family}"]):
            if st != 0 and not (family == "identity" and st == 3):
                raise RuntimeError(f"MotEvaluator: sequence {facts[s]['name']!r}: {family} stopped with status {int(st)} ({_STATUS.get(int(st), 'unknown')})")
    out = {}
    for s, fact in enumerate(facts):
        hf, hi = got["hota_f64"][s], got["hota_i64"][s]
        m = hota_final({"LocA_sum": hf[0], "AssA": hf[1], "AssRe": hf[2], "AssPr": hf[3], "HOTA_TP": hi[0], "HOTA_FN": hi[1], "HOTA_FP": hi[2]})
        del m["LocA_sum"]
        empty = fact["n_pr"] == 0 or fact["n_gt"] == 0
        clear = dict(zip(_CLEAR_INT, (int(v) for v in got["clear_i64"][s])))
        clear["MOTP_sum"], clear["CLR_Frames"] = float(got["clear_f64"][s]), fact["frames"]
        if empty:                                                   # TrackEval returns before its final fields
            clear = {k: 0 for k in _CLEAR_INT + ("CLR_Frames",)}
            clear.update({k: 0.0 for k in CLEAR_FIELDS if k not in clear})
            clear["MLR"] = 1.0
            if fact["n_pr"] == 0:
                clear["CLR_FN"], clear["ML"] = fact["n_gt"], fact["G"]
            else:
                clear["CLR_FP"] = fact["n_pr"]
            m.update(clear)
        else:
            m.update(clear_final(clear))
        idfn, idfp = (int(v) for v in got["identity_i64"][s])
        if got["status_identity"][s] == 3:
            g0, t0, p0, G, T = arrays["seq_gid"][s], arrays["seq_tid"][s], arrays["seq_pair"][s], fact["G"], fact["T"]
            counts = pm.typed(torch.int32, (scalars["pair_total"],))[p0:p0 + G * T].cpu().numpy().reshape(G, T).astype(np.float64)
            idfn, idfp = _identity_on_host(counts, arrays["gt_count"][g0:g0 + G].astype(np.float64), arrays["pr_count"][t0:t0 + T].astype(np.float64))
        ident = {"IDFN": idfn, "IDFP": idfp, "IDTP": fact["n_gt"] - idfn}
        if empty:
            ident = {"IDTP": 0, "IDFN": fact["n_gt"] if fact["n_pr"] == 0 else 0, "IDFP": fact["n_pr"] if fact["n_gt"] == 0 else 0,
                     "IDR": 0.0, "IDP": 0.0, "IDF1": 0.0}
            m.update(ident)
        else:
            m.update(identity_final(ident))
        m["summary"] = _summary(m)
        out[fact["name"]] = m
    out["COMBINED_SEQ"] = combine_sequences({k: v for k, v in out.items()})
    return out


class MotEvaluator:
    """MotEvaluator(device=None): HOTA, CLEAR (MOTA ...) and Identity (IDF1 ...) of any number of sequences.  `device`: the HIP device that
    evaluates; None takes the current one at get_metrics()."""

    def __init__(self, device=None):
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("MotEvaluator runs on HIP devices only (no CPU fallback)")
        self.reset()

    def reset(self):
        """Forget every frame of every sequence."""
        self._sequences = {}          # name -> [(gt boxes, gt ids, pred boxes, pred ids)], in order of arrival

    def update(self, pred_bboxes, pred_track_ids, target_bboxes, target_track_ids, sequence="sequence_0"):
        """Append frames to `sequence` (the reference's argument order and box format): each argument is a list with one entry per frame —
        boxes [n, 4] x y w h and ids [n] as numpy arrays, lists or torch tensors on any device.  ValueError when the four lists differ in
        length, a frame's boxes and ids differ in length, an id repeats inside a frame or a coordinate is not finite."""
        args = (pred_bboxes, pred_track_ids, target_bboxes, target_track_ids)
        if any(not isinstance(a, (list, tuple)) for a in args):
            raise ValueError("MotEvaluator.update: every argument is a list with one entry per frame")
        if len({len(a) for a in args}) != 1:
            raise ValueError(f"MotEvaluator.update: the four lists hold {[len(a) for a in args]} frames")
        frames = []
        for i, (pb, pi, tb, ti) in enumerate(zip(*args)):
            pb, pi = _boxes(pb, f"pred_bboxes[{i}]"), _ids(pi, f"pred_track_ids[{i}]")
            tb, ti = _boxes(tb, f"target_bboxes[{i}]"), _ids(ti, f"target_track_ids[{i}]")
            if len(pb) != len(pi) or len(tb) != len(ti):
                raise ValueError(f"MotEvaluator.update: frame {i} has {len(pb)} predicted boxes for {len(pi)} ids and {len(tb)} target boxes "
                                 f"for {len(ti)} ids")
            frames.append((tb, ti, pb, pi))
        self._sequences.setdefault(str(sequence), []).extend(frames)

    def get_metrics(self):
        """-> {sequence: {...}, "COMBINED_SEQ": {...}}.  Each entry holds every field of the three families under TrackEval's names: the
        HOTA family (HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA, OWTA, HOTA_TP, HOTA_FN, HOTA_FP) as numpy 19-vectors over alpha,
        the CLEAR and Identity fields as Python numbers, and under "summary" the HOTA family as TrackEval's tables report it (the mean
        over alpha).  One upload and one synchronisation."""
        if not self._sequences:
            raise RuntimeError("MotEvaluator.get_metrics: nothing has been evaluated yet")
        dev = self.device
        if dev is None or dev.index is None:
            if not torch.cuda.is_available():
                raise RuntimeError("MotEvaluator runs on HIP devices only (no CPU fallback)")
            dev = torch.device("cuda", torch.cuda.current_device())
        arrays, scalars, facts = pool(list(self._sequences.items()))
        got, pm, _ = run(arrays, scalars, dev)
        return assemble(got, arrays, scalars, facts, pm)


def evaluate_mot_tracking_sequence(pred_bboxes, pred_track_ids, target_bboxes, target_track_ids, device=None):
    """The reference's function (eval/mot_challenge.py:53): one sequence -> {"HOTA": mean over alpha, "MOTA", "IDF1"}."""
    ev = MotEvaluator(device)
    ev.update(pred_bboxes, pred_track_ids, target_bboxes, target_track_ids)
    m = ev.get_metrics()["sequence_0"]
    return {"HOTA": float(m["HOTA"].mean()), "MOTA": m["MOTA"], "IDF1": m["IDF1"]}
