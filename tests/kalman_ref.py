"""numpy restatement of cnl_track_kalman_f64's rule (include/centernet_gfx950.h, csrc/track_kalman.hip): vectorised over the rows, every
product and sum written out in the header's order — no `@`, no np.dot, no np.sum (BLAS and pairwise sums would pick their own order and may
fuse).  float64 throughout; each numpy operation below is one IEEE operation per row, as on the device."""
import numpy as np


def init(b):
    """Birth: b [n, 4] float32 -> (x [n, 8], P [n, 8, 8])."""
    n = b.shape[0]
    x = np.zeros((n, 8))
    x[:, :4] = b.astype(np.float64)
    wh = (x[:, 2] - x[:, 0], x[:, 3] - x[:, 1])
    P = np.zeros((n, 8, 8))
    for i in range(8):
        sd = wh[i & 1] / (10.0 if i < 4 else 16.0)
        P[:, i, i] = sd * sd
    return x, P


def _sum(terms):
    """The first term, then the others added in ascending order."""
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def update(x, P, z):
    """Measurement update of every row: x [n, 8], P [n, 8, 8] (symmetric), z [n, 4] float32 -> (x, P, ok [n] bool); rows whose pivots are
    not all finite and strictly positive come back unchanged with ok False."""
    z = z.astype(np.float64)
    wh = (x[:, 2] - x[:, 0], x[:, 3] - x[:, 1])
    r, y = [], []
    for i in range(4):
        t = wh[i & 1] / 20.0
        r.append(t * t)
        y.append(z[:, i] - x[:, i])
    c = [[None] * 4 for _ in range(4)]
    L = [[None] * 4 for _ in range(4)]
    d = [None] * 4
    ok = np.ones(x.shape[0], bool)
    for j in range(4):
        for i in range(j, 4):
            v = P[:, i, i] + r[i] if i == j else P[:, i, j]
            if j > 0:
                v = v - _sum([c[i][k] * L[j][k] for k in range(j)])
            c[i][j] = v
        d[j] = c[j][j]
        ok &= np.isfinite(d[j]) & (d[j] > 0.0)
        for i in range(j + 1, 4):
            L[i][j] = c[i][j] / d[j]
    K = [[None] * 4 for _ in range(8)]
    for m in range(8):
        u = [None] * 4
        for i in range(4):
            v = P[:, m, i]
            if i > 0:
                v = v - _sum([L[i][k] * u[k] for k in range(i)])
            u[i] = v
        u = [u[i] / d[i] for i in range(4)]
        for i in range(3, -1, -1):
            v = u[i]
            if i < 3:
                v = v - _sum([L[k][i] * K[m][k] for k in range(i + 1, 4)])
            K[m][i] = v
    xn = np.empty_like(x)
    for m in range(8):
        xn[:, m] = x[:, m] + _sum([K[m][k] * y[k] for k in range(4)])
    Pn = np.empty_like(P)
    for i in range(8):
        W = [P[:, i, j] - _sum([K[i][k] * P[:, k, j] for k in range(4)]) for j in range(8)]
        for j in range(i, 8):
            a = _sum([W[k] * K[j][k] for k in range(4)])
            b = _sum([(K[i][k] * r[k]) * K[j][k] for k in range(4)])
            Pn[:, i, j] = (W[j] - a) + b
            Pn[:, j, i] = Pn[:, i, j]
    xn[~ok] = x[~ok]
    Pn[~ok] = P[~ok]
    return xn, Pn, ok


def predict(x, P):
    """Prediction step of every row -> (x, P)."""
    wh = (x[:, 2] - x[:, 0], x[:, 3] - x[:, 1])
    xn = x.copy()
    for i in range(4):
        xn[:, i] = x[:, i] + x[:, 4 + i]
    Pn = P.copy()
    for i in range(4):
        for j in range(i, 4):
            Pn[:, i, j] = (P[:, i, j] + P[:, j, 4 + i]) + (P[:, i, 4 + j] + P[:, 4 + i, 4 + j])
            Pn[:, j, i] = Pn[:, i, j]
        for j in range(4):
            Pn[:, i, 4 + j] = P[:, i, 4 + j] + P[:, 4 + i, 4 + j]
            Pn[:, 4 + j, i] = Pn[:, i, 4 + j]
    for i in range(8):
        sd = wh[i & 1] / (20.0 if i < 4 else 160.0)
        Pn[:, i, i] = Pn[:, i, i] + sd * sd
    return xn, Pn


def track_kalman(x, P, det_box, src_trk, src_det, flags, T_new, new_box):
    """cnl_track_kalman_f64 with its operands as numpy arrays: x [T_old, 8] / P [T_old, 64] float64 (or None), det_box [*, 4] float32, the
    three int32 lists, new_box [T_new, 4] float32 as cnl_track_apply_f32 left it -> (new_x [T_new, 8], new_P [T_new, 64], new_box, out_box
    [T_new, 4] float64, out_status [T_new] int32); new_box is a copy."""
    src_trk, src_det, flags = (np.asarray(a, np.int32)[:T_new] for a in (src_trk, src_det, flags))
    det_box = np.asarray(det_box, np.float32).reshape(-1, 4)
    new_box = np.array(new_box, np.float32).reshape(T_new, 4)
    nx, nP = np.zeros((T_new, 8)), np.zeros((T_new, 8, 8))
    status = np.zeros(T_new, np.int32)
    old = (src_trk >= 0) & (x is not None)
    born = (src_trk < 0) & (src_det >= 0)
    status[~old & ~born] = 2
    with np.errstate(all="ignore"):
        if old.any():
            nx[old], nP[old] = np.asarray(x, np.float64).reshape(-1, 8)[src_trk[old]], np.asarray(P, np.float64).reshape(-1, 8, 8)[src_trk[old]]
            iu = np.triu_indices(8, 1)
            nP[:, iu[1], iu[0]] = nP[:, iu[0], iu[1]]       # an old P is read as its upper triangle
        m = old & (src_det >= 0)
        if m.any():
            nx[m], nP[m], ok = update(nx[m], nP[m], det_box[src_det[m]])
            status[np.flatnonzero(m)[~ok]] = 1
        if born.any():
            nx[born], nP[born] = init(det_box[src_det[born]])
        wr = (src_det >= 0) & (status != 2)
        new_box[wr] = nx[wr, :4].astype(np.float32)
        out_box = nx[:, :4].copy()
        p = (flags & 1) != 0
        if p.any():
            nx[p], nP[p] = predict(nx[p], nP[p])
    return nx, nP.reshape(T_new, 64), new_box, out_box, status
