"""The rule of cnl_reid_loss_f64 / cnl_reid_loss_grad_f32 (include/centernet_gfx950.h) restated in numpy float64: the re-ID loss of the tracking model
(reference models/fairmot.py:34-61: gather at the box centres, Linear / BatchNorm1d / ReLU / Linear, cross entropy over the track identities), its
analytic gradients and the running statistics after the step.  A plain helper (no fixtures): the host test holds it against goldens recorded from the
reference, the GPU tests hold the kernels against it.

The sums run in (n, g) row order, as the rule fixes them; numpy's matrix products use their own order inside a row, which differs from the kernels' by a
few float64 ulps.  reverse=True takes every sum over rows in the opposite order (how far a tensor moves then is the tests' allowance for the order)."""
import numpy as np

KEYS = ("W1", "gamma", "beta", "running_mean", "running_var", "W2", "b2")
GRADS = ("reid", "W1", "gamma", "beta", "W2", "b2")


def rows_of(boxes, ids, count, H, W, K, stride=4, center="trunc", padded_rows=False, ignore_index=-1):
    """-> state [N, G] (0 none, 1 statistics only, 2 live), x [N, G], y [N, G], skipped"""
    boxes, ids = np.asarray(boxes, np.float64), np.asarray(ids, np.int64)
    N, G = ids.shape
    count = np.clip(np.asarray(count, np.int64), 0, G)
    slot = np.arange(G)[None, :] < count[:, None]
    with np.errstate(all="ignore"):
        cx, cy = (boxes[..., 0] + boxes[..., 2] / 2.0) / float(stride), (boxes[..., 1] + boxes[..., 3] / 2.0) / float(stride)
        x, y = (np.rint(cx), np.rint(cy)) if center == "round" else (np.trunc(cx), np.trunc(cy))
        ok = np.isfinite(boxes).all(-1) & (boxes[..., 2] >= 0) & (boxes[..., 3] >= 0) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1) & (ids >= 0) & (ids < K)
    named = slot & (ids != ignore_index)
    live = named & ok
    state = np.where(live, 2, 0)
    if padded_rows:
        state = np.where(~slot, 1, state)
    xi, yi = np.where(live, x, 0).astype(np.int64), np.where(live, y, 0).astype(np.int64)
    return state, xi, yi, int((named & ~ok).sum())


def _forward(reid, boxes, ids, count, cls, training, stride, center, padded_rows, ignore_index, bn_eps, momentum, reverse):
    reid = np.asarray(reid)
    assert reid.dtype == np.float32
    N, D, H, W = reid.shape
    c = {k: np.asarray(cls[k], np.float32).astype(np.float64) for k in KEYS}
    K = c["W2"].shape[0]
    state, x, y, skipped = rows_of(boxes, ids, count, H, W, K, stride, center, padded_rows, ignore_index)
    G = state.shape[1]
    M = int((state == 2).sum())
    f = dict(N=N, D=D, H=H, W=W, K=K, G=G, M=M, skipped=skipped, c=c, training=bool(training), degenerate=False)
    if training and int((state >= 1).sum()) < 2:
        state = np.zeros_like(state)
        f["degenerate"] = True
    stat = np.flatnonzero(state.reshape(-1) >= 1)
    if reverse:
        stat = stat[::-1]
    sn, sg = stat // G, stat % G
    is_live = state.reshape(-1)[stat] == 2
    E = reid[sn, :, y[sn, sg], x[sn, sg]].astype(np.float64)                 # [Rs, D]
    Hh = E @ c["W1"].T
    Rs = len(stat)
    if training and Rs >= 2:
        mean = Hh.sum(0) / Rs
        var = ((Hh - mean) ** 2).sum(0) / Rs
        new_mean = (1.0 - momentum) * c["running_mean"] + momentum * mean
        new_var = (1.0 - momentum) * c["running_var"] + momentum * (var * Rs / (Rs - 1))
        stepped = 1
    else:
        mean, var = c["running_mean"], c["running_var"]
        new_mean, new_var, stepped = mean, var, 0
    sd = np.sqrt(var + bn_eps)
    xhat = (Hh - mean) / sd
    a = xhat * c["gamma"] + c["beta"]
    z = np.maximum(a, 0.0)
    zl = z[is_live]
    id_l = np.asarray(ids, np.int64).reshape(-1)[stat][is_live]
    logits = zl @ c["W2"].T + c["b2"]
    m = logits.max(1, initial=-np.inf)
    with np.errstate(under="ignore"):
        p_un = np.exp(logits - m[:, None])
    lse = m + np.log(p_un.sum(1))
    ce = lse - logits[np.arange(len(id_l)), id_l]
    f.update(stat=stat, sn=sn, sg=sg, x=x, y=y, is_live=is_live, E=E, Hh=Hh, Rs=Rs, sd=sd, xhat=xhat, a=a, z=z, id_l=id_l, logits=logits, lse=lse, ce=ce,
             new_mean=new_mean, new_var=new_var, stepped=stepped)
    return f


def reid_loss(reid, boxes, ids, count, cls, training=True, stride=4, center="trunc", padded_rows=False, ignore_index=-1, bn_eps=1e-5, momentum=0.1,
              reverse=False):
    """-> {"reid" float, "per_row" [N, G] float64, "num_rows", "correct", "skipped", "stepped", "running_mean64" / "running_var64" after the step}"""
    f = _forward(reid, boxes, ids, count, cls, training, stride, center, padded_rows, ignore_index, bn_eps, momentum, reverse)
    per_row = np.zeros(f["N"] * f["G"])
    per_row[f["stat"][f["is_live"]]] = f["ce"]
    correct = int((f["logits"].argmax(1) == f["id_l"]).sum()) if len(f["id_l"]) else 0
    return {"reid": float(f["ce"].sum() / (f["M"] + 1e-8)), "per_row": per_row.reshape(f["N"], f["G"]), "num_rows": f["M"], "correct": correct,
            "skipped": f["skipped"], "stepped": f["stepped"], "running_mean64": np.array(f["new_mean"]), "running_var64": np.array(f["new_var"])}


def reid_loss_grad(reid, boxes, ids, count, cls, training=True, stride=4, center="trunc", padded_rows=False, ignore_index=-1, bn_eps=1e-5,
                   momentum=0.1, scale=1.0, reverse=False):
    """-> {"reid", "W1", "gamma", "beta", "W2", "b2": float64 gradients of scale * value; "read" [N, H, W] bool: the cells some row reads}"""
    f = _forward(reid, boxes, ids, count, cls, training, stride, center, padded_rows, ignore_index, bn_eps, momentum, reverse)
    c, D, K = f["c"], f["D"], f["K"]
    live = f["is_live"]
    with np.errstate(under="ignore"):
        g = np.exp(f["logits"] - f["lse"][:, None])
    g[np.arange(len(f["id_l"])), f["id_l"]] -= 1.0
    g *= float(scale) / (f["M"] + 1e-8)
    zl = f["z"][live]
    dW2 = g.T @ zl if len(zl) else np.zeros((K, D))
    db2 = g.sum(0)
    dz = np.zeros_like(f["z"])
    dz[live] = g @ c["W2"]
    da = np.where(f["a"] > 0, dz, 0.0)
    da[~live] = 0.0
    dbeta = da.sum(0)
    dgamma = (da * f["xhat"]).sum(0)
    dxhat = da * c["gamma"]
    if f["training"] and f["Rs"] >= 2:
        Rs = f["Rs"]
        dh = (Rs * dxhat - dxhat.sum(0) - f["xhat"] * (dxhat * f["xhat"]).sum(0)) / (Rs * f["sd"])
    else:
        dh = dxhat / f["sd"]
    dW1 = dh.T @ f["E"] if f["Rs"] else np.zeros((D, D))
    de = dh @ c["W1"]
    d_reid = np.zeros((f["N"], D, f["H"], f["W"]))
    read = np.zeros((f["N"], f["H"], f["W"]), bool)
    for i in range(f["Rs"]):                                                  # row order (or its reverse)
        n, yy, xx = f["sn"][i], f["y"][f["sn"][i], f["sg"][i]], f["x"][f["sn"][i], f["sg"][i]]
        d_reid[n, :, yy, xx] += de[i]
        read[n, yy, xx] = True
    return {"reid": d_reid, "W1": dW1, "gamma": dgamma, "beta": dbeta, "W2": dW2, "b2": db2, "read": read}
