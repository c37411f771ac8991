"""TEST INFRASTRUCTURE — a pure-Python restatement of the assignment algorithm csrc/track_streams.hip is written against:
scipy.optimize.linear_sum_assignment's rectangular shortest augmenting path (Crouse 2016, scipy/optimize/rectangular_lsap) in scipy's
order and in float64, with the scan over the remaining columns expressed the way the kernel runs it: `lanes` lanes each walk the
positions it = lane, lane + lanes, ... in ascending order with scipy's own condition, and the per-lane candidates are merged by the key

    lower cost first;  at equal cost an unassigned column before an assigned one;
    among unassigned columns the LARGEST position `it`;  among assigned columns the SMALLEST

which reproduces the sequential rule `spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1)`.  tests/test_track_streams_host.py
holds this against scipy itself (rows and columns, ties included), which pins the specification on the CPU; the GPU tests hold the
kernel against scipy directly."""
import math

import numpy as np

INVALID, INFEASIBLE = "invalid", "infeasible"


def _better(a, b):
    """Is candidate a = (cost, free, it) ahead of b in the merge order?"""
    if a[0] != b[0]:
        return a[0] < b[0]
    if a[1] != b[1]:
        return a[1]
    return a[2] > b[2] if a[1] else a[2] < b[2]


def _solve(cost, nr, nc, lanes):
    """cost[i][j], nr <= nc -> (col4row, row4col) or a status string."""
    inf = math.inf
    u, v = [0.0] * nr, [0.0] * nc
    path, row4col, col4row = [-1] * nc, [-1] * nc, [-1] * nr
    for cur in range(nr):
        remaining = [nc - it - 1 for it in range(nc)]
        spc = [inf] * nc
        min_val, num_remaining, sink, i = 0.0, nc, -1, cur
        while sink == -1:
            cands = []
            for lane in range(lanes):
                best = (inf, False, -1)
                for it in range(lane, num_remaining, lanes):
                    j = remaining[it]
                    r = ((min_val + cost[i][j]) - u[i]) - v[j]
                    if r < spc[j]:
                        path[j] = i
                        spc[j] = r
                    free = row4col[j] == -1
                    if spc[j] < best[0] or (spc[j] == best[0] and free):
                        best = (spc[j], free, it)
                cands.append(best)
            best = cands[0]
            for c in cands[1:]:
                if _better(c, best):
                    best = c
            min_val = best[0]
            if min_val == inf:
                return INFEASIBLE
            index = best[2]
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
            remaining[num_remaining] = j            # parked behind the live part: the scanned columns, as the kernel keeps them
        u[cur] = u[cur] + min_val
        for idx in range(num_remaining, nc):
            j = remaining[idx]
            d = min_val - spc[j]
            if row4col[j] != -1:
                u[row4col[j]] = u[row4col[j]] + d
            v[j] = v[j] - d
        j = sink
        while True:
            pi = path[j]
            row4col[j] = pi
            col4row[pi], j = j, col4row[pi]
            if pi == cur:
                break
    return col4row, row4col


def linear_sum_assignment(cost, lanes=64):
    """(row_ind, col_ind) as scipy returns them, or raises ValueError where scipy does."""
    c = np.asarray(cost, dtype=np.float64)
    n, T = c.shape
    if n == 0 or T == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if np.isnan(c).any() or np.isneginf(c).any():
        raise ValueError("matrix contains invalid numeric entries")
    transposed = n > T
    m = (c.T if transposed else c).tolist()
    res = _solve(m, min(n, T), max(n, T), lanes)
    if res == INFEASIBLE:
        raise ValueError("cost matrix is infeasible")
    col4row, row4col = res
    if transposed:
        per_row = np.asarray(row4col, np.int64)                # original row -> original column or -1
        rows = np.flatnonzero(per_row >= 0)
        return rows, per_row[rows]
    return np.arange(n, dtype=np.int64), np.asarray(col4row, np.int64)


def matrices(kind, n, T, rng):
    """The four kinds of matrix the assignment tests use."""
    if kind == "uniform":
        return rng.random((n, T))
    if kind == "ties":
        return rng.integers(0, 4, (n, T)).astype(np.float64)
    if kind == "iou":                                            # IoU-like: 1.0 except ~15 % float32 values below 1
        m = np.ones((n, T), np.float32)
        hit = rng.random((n, T)) < 0.15
        m[hit] = rng.random(int(hit.sum())).astype(np.float32)
        return m.astype(np.float64)
    if kind == "decimal":
        return np.round(rng.random((n, T)), 1)
    raise ValueError(kind)


KINDS = ("uniform", "ties", "iou", "decimal")
