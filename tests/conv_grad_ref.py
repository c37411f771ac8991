"""The convolution gradients of csrc/conv_grad.hip restated in numpy float64, and the gradients of the BatchNorm fold.  A plain helper (no tests)
for tests/test_conv_grad_host.py (which holds it against torch's float64 autograd) and tests/test_gpu_conv_grad.py.

Tensors are logical NCHW here; weights are OHWI [Cout, K, K, Cin], the engine's layout.  The layer is  z = conv(x, w) + b (stride 1, pad K // 2),
y = relu(z);  dy is the loss gradient with respect to y."""
import numpy as np

WG_CO, WG_CI, WG_TARGET, WG_MIN_PIX = 128, 32, 1024, 512      # the slice function's constants (include/centernet_gfx950.h)
RG_PIX = 256                                                  # pixels a workgroup of cnl_relu_grad_f32 owns
U = 2.0 ** -24                                                # fp32 unit roundoff


def ceil_div(a, b):
    return -(-a // b)


def wgrad_geometry(N, H, W, Cin, Cout, K):
    """The header's slice function -> {"slices", "rows_per_slice", "workspace_bytes", "terms"}"""
    tiles = ceil_div(Cout, WG_CO) * (Cin // WG_CI)
    rows = N * H
    rps = min(rows, max(ceil_div(rows, ceil_div(WG_TARGET, tiles)), ceil_div(WG_MIN_PIX, W)))
    slices = ceil_div(rows, rps)
    return {"slices": slices, "rows_per_slice": rps, "workspace_bytes": slices * Cout * K * K * Cin * 4, "terms": rps * W + slices}


def relu_grad_workspace_bytes(N, C, H, W):
    return ceil_div(N * H * W, RG_PIX) * C * 4


def relu_grad(dy, y=None):
    """-> (dz = dy where y > 0 else 0 (y None: dy), dbias [C] = sum of dz over n, h, w)"""
    dy = np.asarray(dy, np.float64)
    dz = dy.copy() if y is None else np.where(np.asarray(y) > 0, dy, 0.0)
    return dz, dz.sum(axis=(0, 2, 3))


def dbias_as_the_kernel_sums(dz32, C):
    """dbias in the kernel's own order, for a float32 dz [N, C, H, W]: workgroups of 256 consecutive pixels; cpt = min(256, C rounded up to a power of
    two) threads per pixel, 256 / cpt pixel lanes with stride 256 / cpt, each lane in pixel order in fp32, the lanes in lane order in fp32, the
    workgroups in float64, rounded once."""
    flat = np.ascontiguousarray(np.asarray(dz32, np.float32).transpose(0, 2, 3, 1)).reshape(-1, C)
    cpt = 1
    while cpt < C and cpt < 256:
        cpt *= 2
    pl = 256 // cpt
    total = np.zeros(C, np.float64)
    for p0 in range(0, flat.shape[0], RG_PIX):
        blk = flat[p0:p0 + RG_PIX]
        lanes = np.zeros((pl, C), np.float32)
        for j in range(blk.shape[0]):
            lanes[j % pl] = lanes[j % pl] + blk[j]
        s = lanes[0].copy()
        for j in range(1, pl):
            s = s + lanes[j]
        total += s.astype(np.float64)
    return total.astype(np.float32)


def wgrad(x, dz, K):
    """dW[co][ky][kx][ci] = sum_{n, oy, ox} dz[n, co, oy, ox] x[n, ci, oy + ky - K // 2, ox + kx - K // 2], zero outside the image"""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    N, Cin, H, W = x.shape
    pad = K // 2
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    dw = np.zeros((dz.shape[1], K, K, Cin))
    for ky in range(K):
        for kx in range(K):
            dw[:, ky, kx, :] = np.einsum("nohw,nihw->oi", dz, xp[:, :, ky:ky + H, kx:kx + W])
    return dw


def dgrad(dz, w_ohwi):
    """dx[n, ci, iy, ix] = sum_{co, ky, kx} dz[n, co, iy - ky + pad, ix - kx + pad] w[co][ky][kx][ci], zero outside the image"""
    dz, w = np.asarray(dz, np.float64), np.asarray(w_ohwi, np.float64)
    N, Cout, H, W = dz.shape
    K = w.shape[1]
    pad = K // 2
    zp = np.pad(dz, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    dx = np.zeros((N, w.shape[3], H, W))
    for ky in range(K):
        for kx in range(K):
            dx += np.einsum("nohw,oi->nihw", zp[:, :, 2 * pad - ky:2 * pad - ky + H, 2 * pad - kx:2 * pad - kx + W], w[:, ky, kx, :])
    return dx


def conv(x, w_ohwi, b=None, relu=False):
    """The forward layer in float64."""
    x, w = np.asarray(x, np.float64), np.asarray(w_ohwi, np.float64)
    N, Cin, H, W = x.shape
    K = w.shape[1]
    pad = K // 2
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    z = np.zeros((N, w.shape[0], H, W))
    for ky in range(K):
        for kx in range(K):
            z += np.einsum("nihw,oi->nohw", xp[:, :, ky:ky + H, kx:kx + W], w[:, ky, kx, :])
    if b is not None:
        z += np.asarray(b, np.float64).reshape(1, -1, 1, 1)
    return np.maximum(z, 0.0) if relu else z


def fold(weight_oihw, gamma, beta, mean, var, eps):
    """Eval-mode BatchNorm folded into a bias-free conv -> (W' OHWI, b')"""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    w = np.asarray(weight_oihw, np.float64) * scale.reshape(-1, 1, 1, 1)
    return w.transpose(0, 2, 3, 1), np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale


def fold_grad(dw_ohwi, db, weight_oihw, gamma, mean, var, eps):
    """The folded gradients carried back: W' = W gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps)
    -> (dweight OIHW, dgamma, dbeta)"""
    inv = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    dwp = np.asarray(dw_ohwi, np.float64).transpose(0, 3, 1, 2)
    weight = np.asarray(weight_oihw, np.float64)
    dweight = dwp * (np.asarray(gamma, np.float64) * inv).reshape(-1, 1, 1, 1)
    dgamma = ((dwp * weight).sum(axis=(1, 2, 3)) - np.asarray(mean, np.float64) * np.asarray(db, np.float64)) * inv
    return dweight, dgamma, np.asarray(db, np.float64).copy()


# (N, H, W, Cin, Cout, K) of the kernel tests: the smallest shapes that cross every seam — W = 19 and 65 are odd (a pixel pair with one live pixel), 65
# crosses the 64-pixel chunk, 2 x 9 rows of 64 pixels give three slices with a short last one, 3 x 5 x 19 and 1 x 1 x 1 are smaller than a slice, Cout = 80 /
# 96 leave a wave of the 128-cout tile partly / wholly idle and 160 crosses into a second tile, Cin = 64 / 96 give two / three channel slices
CASES = [(3, 5, 19, 32, 1, 3), (3, 5, 19, 64, 2, 1), (1, 1, 1, 32, 4, 3), (1, 1, 1, 96, 80, 1), (2, 9, 64, 32, 1, 3), (2, 9, 64, 96, 96, 3),
         (2, 8, 65, 64, 80, 3), (2, 8, 65, 32, 96, 1), (3, 5, 19, 96, 4, 3), (2, 9, 64, 64, 2, 1), (2, 8, 65, 96, 1, 1), (3, 5, 19, 32, 80, 3),
         (2, 9, 64, 64, 160, 3)]


def case_tensors(case, seed=0):
    """x, dy, y-sign pattern and weights of a case, float32 numpy (logical NCHW / OHWI), drawn from the case and the seed alone."""
    N, H, W, Cin, Cout, K = case
    rng = np.random.default_rng([seed, N, H, W, Cin, Cout, K])
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    dy = (rng.standard_normal((N, Cout, H, W)) * np.exp(rng.uniform(-6, 2, (N, Cout, H, W)))).astype(np.float32)      # spans decades, as a loss gradient does
    w = (rng.standard_normal((Cout, K, K, Cin)) / np.sqrt(K * K * Cin)).astype(np.float32)
    return x, dy, w
