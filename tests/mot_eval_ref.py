"""The tracking evaluation's rule (include/centernet_gfx950.h: TrackEval's HOTA, CLEAR and Identity for MotChallenge2DBox on the data the
reference's writer produces) restated in numpy + scipy, sequence by sequence, with the summation orders the header fixes: every sum is
a Python loop of single float64 additions, so the device's results can be compared with these bit for bit.  TrackEval is not available;
tests/test_mot_eval_host.py pins this restatement on hand-worked cases.

A sequence is a list of frames (gt_boxes [n, 4] x y w h, gt_ids [n], pred_boxes [m, 4], pred_ids [m]).
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = np.finfo("float").eps
ALPHA = np.arange(0.05, 0.99, 0.05)
solves = []        # (cost matrix, rows, cols) of every assignment solved since the last clear(): what test 4 inspects


def solve(cost):
    rows, cols = linear_sum_assignment(cost)
    solves.append((cost.copy(), rows.copy(), cols.copy()))
    return rows, cols


def similarity(g, d):
    """[n, 4] and [m, 4] x y w h -> [n, m]"""
    g, d = np.asarray(g, np.float64).reshape(-1, 4), np.asarray(d, np.float64).reshape(-1, 4)
    x0g, y0g, x1g, y1g = g[:, 0, None], g[:, 1, None], (g[:, 0] + g[:, 2])[:, None], (g[:, 1] + g[:, 3])[:, None]
    x0d, y0d, x1d, y1d = d[None, :, 0], d[None, :, 1], (d[:, 0] + d[:, 2])[None, :], (d[:, 1] + d[:, 3])[None, :]
    iw = np.maximum(np.minimum(x1g, x1d) - np.maximum(x0g, x0d), 0.0)
    ih = np.maximum(np.minimum(y1g, y1d) - np.maximum(y0g, y0d), 0.0)
    inter = iw * ih
    ag, ad = (x1g - x0g) * (y1g - y0g), (x1d - x0d) * (y1d - y0d)
    union = (ag + ad) - inter
    zero = (ag <= EPS) | (ad <= EPS) | (union <= EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = inter / union
    return np.where(zero, 0.0, s)


def seq_sum(values):
    """Sequential float64 sum from 0.0."""
    acc = np.float64(0.0)
    for v in values:
        acc = acc + np.float64(v)
    return acc


def prepare(frames):
    """Relabel both sides to 0..n-1 in ascending order of the original id -> dict with per-frame ids, similarities and the counts."""
    def relabel(id_frames):
        flat = np.concatenate([np.asarray(i, np.int64).reshape(-1) for i in id_frames]) if id_frames else np.zeros(0, np.int64)
        unique = np.unique(flat)
        for i in id_frames:
            if len(np.unique(np.asarray(i))) != len(np.asarray(i).reshape(-1)):
                raise ValueError("an id repeats inside one frame")
        return [np.searchsorted(unique, np.asarray(i, np.int64).reshape(-1)) for i in id_frames], len(unique)
    gt_ids, G = relabel([f[1] for f in frames])
    tr_ids, T = relabel([f[3] for f in frames])
    sims = [similarity(f[0], f[2]) for f in frames]
    return {"gt_ids": gt_ids, "tr_ids": tr_ids, "G": G, "T": T, "sim": sims, "n_gt": sum(len(i) for i in gt_ids), "n_tr": sum(len(i) for i in tr_ids),
            "frames": len(frames)}


# ---------------------------------------------------------------------------------------------------------------- HOTA
def hota_final(res):
    tp, fn, fp = (np.asarray(res[k], np.float64) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP"))
    res["DetRe"] = tp / np.maximum(1.0, tp + fn)
    res["DetPr"] = tp / np.maximum(1.0, tp + fp)
    res["DetA"] = tp / np.maximum(1.0, tp + fn + fp)
    res["HOTA"] = np.sqrt(res["DetA"] * res["AssA"])
    res["OWTA"] = np.sqrt(res["DetRe"] * res["AssA"])
    return res


def hota(data):
    n = len(ALPHA)
    res = {k: np.zeros(n) for k in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA", "OWTA")}
    res.update({k: np.zeros(n, np.int64) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP")})
    if data["n_tr"] == 0:
        res["HOTA_FN"][:] = data["n_gt"]
        res["LocA"][:] = 1.0
        return res
    if data["n_gt"] == 0:
        res["HOTA_FP"][:] = data["n_tr"]
        res["LocA"][:] = 1.0
        return res
    G, T = data["G"], data["T"]
    potential, gt_count, trk_count = np.zeros((G, T)), np.zeros(G), np.zeros(T)
    for gids, tids, s in zip(data["gt_ids"], data["tr_ids"], data["sim"]):
        r = [seq_sum(s[i, :]) for i in range(len(gids))]
        c = [seq_sum(s[:, j]) for j in range(len(tids))]
        for i, g in enumerate(gids):
            for j, t in enumerate(tids):
                den = (c[j] + r[i]) - s[i, j]
                sim_iou = s[i, j] / den if den > EPS else 0.0
                potential[g, t] = potential[g, t] + sim_iou
        gt_count[gids] += 1
        trk_count[tids] += 1
    gas = potential / ((gt_count[:, None] + trk_count[None, :]) - potential)
    matches = np.zeros((n, G, T), np.int64)
    loc_sum = np.zeros(n)
    for gids, tids, s in zip(data["gt_ids"], data["tr_ids"], data["sim"]):
        if len(gids) == 0:
            res["HOTA_FP"] += len(tids)
            continue
        if len(tids) == 0:
            res["HOTA_FN"] += len(gids)
            continue
        score = gas[gids[:, None], tids[None, :]] * s
        rows, cols = solve(-score)
        for a, alpha in enumerate(ALPHA):
            frame_sum, count = np.float64(0.0), 0
            for i, j in sorted(zip(rows, cols)):
                if s[i, j] >= alpha - EPS:
                    frame_sum = frame_sum + s[i, j]
                    count += 1
                    matches[a, gids[i], tids[j]] += 1
            res["HOTA_TP"][a] += count
            res["HOTA_FN"][a] += len(gids) - count
            res["HOTA_FP"][a] += len(tids) - count
            loc_sum[a] = loc_sum[a] + frame_sum
    for a in range(n):
        m = matches[a].astype(np.float64)
        for key, den in (("AssA", np.maximum(1.0, (gt_count[:, None] + trk_count[None, :]) - m)), ("AssRe", np.maximum(1.0, gt_count[:, None]) + 0 * m),
                         ("AssPr", np.maximum(1.0, trk_count[None, :]) + 0 * m)):
            term = m * (m / den)
            rows_sum = seq_sum(seq_sum(term[g, term[g] != 0]) for g in range(G))      # (a zero adds +0.0: skipped)
            res[key][a] = rows_sum / np.maximum(1.0, np.float64(res["HOTA_TP"][a]))
    res["LocA"] = np.maximum(1e-10, loc_sum) / np.maximum(1e-10, res["HOTA_TP"].astype(np.float64))
    return hota_final(res)


# ---------------------------------------------------------------------------------------------------------------- CLEAR
CLEAR_INT = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "CLR_Frames")
CLEAR_FLOAT = ("MOTA", "MOTP", "MODA", "CLR_Re", "CLR_Pr", "MTR", "PTR", "MLR", "sMOTA", "CLR_F1", "FP_per_frame", "MOTAL", "MOTP_sum")


def clear_final(res):
    tp, fn, fp, idsw = (np.float64(res[k]) for k in ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW"))
    ids = np.float64(res["MT"] + res["ML"] + res["PT"])
    res["MTR"] = float(res["MT"] / np.maximum(1.0, ids))
    res["MLR"] = float(res["ML"] / np.maximum(1.0, ids))
    res["PTR"] = float(res["PT"] / np.maximum(1.0, ids))
    res["CLR_Re"] = float(tp / np.maximum(1.0, tp + fn))
    res["CLR_Pr"] = float(tp / np.maximum(1.0, tp + fp))
    res["MODA"] = float((tp - fp) / np.maximum(1.0, tp + fn))
    res["MOTA"] = float((tp - fp - idsw) / np.maximum(1.0, tp + fn))
    res["MOTP"] = float(res["MOTP_sum"] / np.maximum(1.0, tp))
    res["sMOTA"] = float((res["MOTP_sum"] - fp - idsw) / np.maximum(1.0, tp + fn))
    res["CLR_F1"] = float(tp / np.maximum(1.0, tp + 0.5 * fn + 0.5 * fp))
    res["FP_per_frame"] = float(fp / np.maximum(1.0, np.float64(res["CLR_Frames"])))
    safe_log_idsw = np.log10(idsw) if idsw > 0 else idsw
    res["MOTAL"] = float((tp - fp - safe_log_idsw) / np.maximum(1.0, tp + fn))
    return res


def clear(data, trace=None):
    """trace: a list that receives prev_step (a copy, NaN = none) after every frame."""
    res = {k: 0 for k in CLEAR_INT}
    res.update({k: 0.0 for k in CLEAR_FLOAT})
    if data["n_tr"] == 0:
        res["CLR_FN"], res["ML"], res["MLR"] = data["n_gt"], data["G"], 1.0
        return res
    if data["n_gt"] == 0:
        res["CLR_FP"], res["MLR"] = data["n_tr"], 1.0
        return res
    G = data["G"]
    gt_count, matched_count, frag_count = np.zeros(G), np.zeros(G), np.zeros(G)
    prev, prev_step = np.full(G, np.nan), np.full(G, np.nan)
    motp = np.float64(0.0)
    for gids, tids, s in zip(data["gt_ids"], data["tr_ids"], data["sim"]):
        if len(gids) == 0:
            res["CLR_FP"] += len(tids)
        elif len(tids) == 0:
            res["CLR_FN"] += len(gids)
            gt_count[gids] += 1
        else:
            score = 1000 * (tids[None, :] == prev_step[gids[:, None]]) + s
            score[s < 0.5 - EPS] = 0
            rows, cols = solve(-score)
            keep = score[rows, cols] > 0 + EPS
            rows, cols = rows[keep], cols[keep]
            m_g, m_t = gids[rows], tids[cols]
            before = prev[m_g]
            res["IDSW"] += int(np.sum(~np.isnan(before) & (m_t != before)))
            gt_count[gids] += 1
            matched_count[m_g] += 1
            was_none = np.isnan(prev_step)
            prev[m_g] = m_t
            prev_step[:] = np.nan
            prev_step[m_g] = m_t
            frag_count += was_none & ~np.isnan(prev_step)
            res["CLR_TP"] += len(m_g)
            res["CLR_FN"] += len(gids) - len(m_g)
            res["CLR_FP"] += len(tids) - len(m_g)
            motp = motp + seq_sum(s[i, j] for i, j in sorted(zip(rows, cols)))
        if trace is not None:
            trace.append(prev_step.copy())
    ratio = matched_count[gt_count > 0] / gt_count[gt_count > 0]
    res["MT"] = int(np.sum(ratio > 0.8))
    res["PT"] = int(np.sum(ratio >= 0.2)) - res["MT"]
    res["ML"] = G - res["MT"] - res["PT"]
    res["Frag"] = int(np.sum(frag_count[frag_count > 0] - 1))
    res["MOTP_sum"] = float(motp)
    res["CLR_Frames"] = data["frames"]
    return clear_final(res)


# ---------------------------------------------------------------------------------------------------------------- Identity
def identity_final(res):
    tp, fn, fp = (np.float64(res[k]) for k in ("IDTP", "IDFN", "IDFP"))
    res["IDR"] = float(tp / np.maximum(1.0, tp + fn))
    res["IDP"] = float(tp / np.maximum(1.0, tp + fp))
    res["IDF1"] = float(tp / np.maximum(1.0, tp + 0.5 * fp + 0.5 * fn))
    return res


def identity(data):
    res = {"IDTP": 0, "IDFN": 0, "IDFP": 0, "IDF1": 0.0, "IDR": 0.0, "IDP": 0.0}
    if data["n_tr"] == 0:
        res["IDFN"] = data["n_gt"]
        return res
    if data["n_gt"] == 0:
        res["IDFP"] = data["n_tr"]
        return res
    G, T = data["G"], data["T"]
    pm, gt_count, trk_count = np.zeros((G, T)), np.zeros(G), np.zeros(T)
    for gids, tids, s in zip(data["gt_ids"], data["tr_ids"], data["sim"]):
        i, j = np.nonzero(s >= 0.5)
        pm[gids[i], tids[j]] += 1
        gt_count[gids] += 1
        trk_count[tids] += 1
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fp[G:, :T] = 1e10
    fn[:G, T:] = 1e10
    for g in range(G):
        fn[g, :T] = gt_count[g]
        fn[g, T + g] = gt_count[g]
    for t in range(T):
        fp[:G, t] = trk_count[t]
        fp[G + t, t] = trk_count[t]
    fn[:G, :T] -= pm
    fp[:G, :T] -= pm
    rows, cols = solve(fn + fp)
    res["IDFN"] = int(fn[rows, cols].sum())
    res["IDFP"] = int(fp[rows, cols].sum())
    res["IDTP"] = int(gt_count.sum()) - res["IDFN"]
    return identity_final(res)


# ---------------------------------------------------------------------------------------------------------------- all
def evaluate_sequence(frames):
    data = prepare(frames)
    out = hota(data)
    out.update(clear(data))
    out.update(identity(data))
    return out


def combine(per_sequence):
    """[metrics] in order -> COMBINED_SEQ"""
    res = {k: sum(m[k] for m in per_sequence) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP")}
    tp = res["HOTA_TP"].astype(np.float64)
    for k in ("AssRe", "AssPr", "AssA"):
        acc = np.zeros(len(ALPHA))
        for m in per_sequence:
            acc = acc + m[k] * m["HOTA_TP"]
        res[k] = acc / np.maximum(1.0, tp)
    acc = np.zeros(len(ALPHA))
    for m in per_sequence:
        acc = acc + m["LocA"] * m["HOTA_TP"]
    res["LocA"] = np.maximum(1e-10, acc) / np.maximum(1e-10, tp)
    res = hota_final(res)
    for k in CLEAR_INT:
        res[k] = sum(m[k] for m in per_sequence)
    res["MOTP_sum"] = float(seq_sum(m["MOTP_sum"] for m in per_sequence))
    clear_final(res)
    for k in ("IDTP", "IDFN", "IDFP"):
        res[k] = sum(m[k] for m in per_sequence)
    return identity_final(res)


def evaluate(sequences):
    """{name: frames} -> {name: metrics, "COMBINED_SEQ": metrics}"""
    out = {name: evaluate_sequence(frames) for name, frames in sequences.items()}
    out["COMBINED_SEQ"] = combine(list(out.values()))
    return out


def evaluate_mot_tracking_sequence(pred_bboxes, pred_track_ids, target_bboxes, target_track_ids):
    m = evaluate_sequence(list(zip(target_bboxes, target_track_ids, pred_bboxes, pred_track_ids)))
    return {"HOTA": float(m["HOTA"].mean()), "MOTA": m["MOTA"], "IDF1": m["IDF1"]}
