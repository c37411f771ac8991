"""The conv-gradient family without a GPU: the symbols, every refusal, the pure host queries against the stated formula, and the numpy float64
restatement (tests/conv_grad_ref.py) against torch's float64 CPU autograd of F.conv2d + ReLU (+ eval-mode BatchNorm2d) on the shapes the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as G
from centernet_lightning_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cnl_relu_grad_workspace_bytes", "cnl_relu_grad_terms", "cnl_relu_grad_f32", "cnl_conv_wgrad_slices", "cnl_conv_wgrad_workspace_bytes",
           "cnl_conv_wgrad_terms", "cnl_conv_wgrad_nhwc_f32", "cnl_conv1x1_dgrad_nhwc_f32")
A = 1 << 20          # a 16-byte aligned, never dereferenced "pointer": every refusal below happens before anything is launched


def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert lib.cnl_version() == 13 and _lib.ABI_VERSION == 13
    assert lib.cnl_sizeof_params(3) == 0
    assert lib.cnl_sizeof_params(0) == ctypes.sizeof(_lib.ConvParams)


def wgrad(lib, x=A, ldx=32, dz=A, lddz=4, dw=A, N=1, H=4, W=4, Cin=32, Cout=4, KH=3, KW=3, pad=1, ws=A, ws_bytes=1 << 30):
    return lib.cnl_conv_wgrad_nhwc_f32(x, ldx, dz, lddz, dw, N, H, W, Cin, Cout, KH, KW, pad, ws, ws_bytes, None)


def relu(lib, dy=A, strides=(64, 1, 16, 4), y=A, ldy=4, N=1, C=4, H=4, W=4, dz=A, lddz=4, dbias=A, ws=A, ws_bytes=1 << 20):
    return lib.cnl_relu_grad_f32(dy, *strides, y, ldy, N, C, H, W, dz, lddz, dbias, ws, ws_bytes, None)


def dgrad(lib, dz=A, lddz=4, w=A, dx=A, lddx=32, N=1, H=4, W=4, Cin=32, Cout=4):
    return lib.cnl_conv1x1_dgrad_nhwc_f32(dz, lddz, w, dx, lddx, N, H, W, Cin, Cout, None)


BAD, UNS, WSP = _lib.CNL_E_BAD_ARG, _lib.CNL_E_UNSUPPORTED, _lib.CNL_E_WORKSPACE
REFUSALS = [
    (wgrad, dict(x=None), BAD, "null"), (wgrad, dict(dz=None), BAD, "null"), (wgrad, dict(dw=None), BAD, "null"),
    (wgrad, dict(N=0), BAD, "non-positive"), (wgrad, dict(H=-1), BAD, "non-positive"), (wgrad, dict(Cout=0), BAD, "non-positive"),
    (wgrad, dict(KH=5, KW=5, pad=2), UNS, "kernel"), (wgrad, dict(KH=3, KW=1), UNS, "kernel"), (wgrad, dict(pad=0), UNS, "pad"),
    (wgrad, dict(KH=1, KW=1, pad=1), UNS, "pad"), (wgrad, dict(Cin=48, ldx=48), UNS, "multiple of 32"),
    (wgrad, dict(ldx=16), BAD, "ldx"), (wgrad, dict(ldx=34), BAD, "ldx"), (wgrad, dict(x=A + 4), BAD, "16-byte"),
    (wgrad, dict(lddz=2), BAD, "lddz"), (wgrad, dict(lddz=6), BAD, "lddz"), (wgrad, dict(dz=A + 8), BAD, "16-byte"), (wgrad, dict(dw=A + 4), BAD, "16-byte"),
    (wgrad, dict(N=32768, H=1024, W=1024), UNS, "4 GiB"),
    (wgrad, dict(ws=None), WSP, "workspace"), (wgrad, dict(ws_bytes=16), WSP, "workspace"), (wgrad, dict(ws=A + 4), BAD, "workspace"),
    (relu, dict(dy=None), BAD, "null"), (relu, dict(dz=None), BAD, "null"), (relu, dict(C=0), BAD, "non-positive"), (relu, dict(W=0), BAD, "non-positive"),
    (relu, dict(strides=(64, -1, 16, 4)), BAD, "stride"), (relu, dict(lddz=2), BAD, "lddz"), (relu, dict(lddz=5, C=5), BAD, "lddz"),
    (relu, dict(dz=A + 4), BAD, "16-byte"), (relu, dict(ldy=3), BAD, "ldy"), (relu, dict(dy=A + 2), BAD, "4-byte"), (relu, dict(y=A + 1), BAD, "4-byte"),
    (relu, dict(N=32768, H=1024, W=1024), UNS, "4 GiB"), (relu, dict(ws=None), WSP, "workspace"), (relu, dict(ws_bytes=8), WSP, "workspace"),
    (dgrad, dict(dz=None), BAD, "null"), (dgrad, dict(w=None), BAD, "null"), (dgrad, dict(dx=None), BAD, "null"), (dgrad, dict(Cout=0), BAD, "non-positive"),
    (dgrad, dict(Cin=16, lddx=16), UNS, "multiple of 32"), (dgrad, dict(lddz=3), BAD, "lddz"), (dgrad, dict(lddx=28), BAD, "lddx"),
    (dgrad, dict(lddx=33), BAD, "lddx"), (dgrad, dict(dx=A + 4), BAD, "16-byte"), (dgrad, dict(dz=A + 12), BAD, "16-byte"), (dgrad, dict(w=A + 4), BAD, "16-byte"),
    (dgrad, dict(N=32768, H=1024, W=1024), UNS, "4 GiB"),
]


@pytest.mark.parametrize("call,kw,code,text", REFUSALS, ids=[f"{c.__name__}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for c, kw, _, _ in REFUSALS])
def test_every_refusal_returns_its_code_without_a_gpu(call, kw, code, text):
    lib = _lib.load()
    assert call(lib, **kw) == code
    assert text in _lib.last_error(), _lib.last_error()


SHAPES = G.CASES + [(32, 128, 128, 64, 256, 3), (32, 128, 128, 256, 256, 3), (32, 128, 128, 256, 80, 1), (32, 152, 272, 256, 256, 3), (1, 7, 3, 32, 1000, 1),
                    (2, 2, 4096, 32, 4, 3)]


@pytest.mark.parametrize("case", SHAPES, ids=[",".join(map(str, c)) for c in SHAPES])
def test_host_queries_follow_the_stated_formula(case):
    lib = _lib.load()
    N, H, W, Cin, Cout, K = case
    g = G.wgrad_geometry(N, H, W, Cin, Cout, K)
    assert lib.cnl_conv_wgrad_slices(N, H, W, Cin, Cout, K, K) == g["slices"]
    assert lib.cnl_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout, K, K) == g["workspace_bytes"]
    assert lib.cnl_conv_wgrad_terms(N, H, W, Cin, Cout, K, K) == g["terms"]
    assert (g["slices"] - 1) * g["rows_per_slice"] < N * H <= g["slices"] * g["rows_per_slice"]
    assert lib.cnl_relu_grad_workspace_bytes(N, Cout, H, W) == G.relu_grad_workspace_bytes(N, Cout, H, W)
    assert lib.cnl_relu_grad_terms(N, Cout, H, W) == G.RG_PIX + 1


def test_host_queries_answer_zero_for_what_the_entry_refuses():
    lib = _lib.load()
    for args in ((0, 4, 4, 32, 4, 3, 3), (1, 4, 4, 48, 4, 3, 3), (1, 4, 4, 32, 4, 5, 5), (1, 4, 4, 32, 0, 1, 1), (1, 4, 4, 32, 4, 3, 1)):
        assert lib.cnl_conv_wgrad_slices(*args) == 0 and lib.cnl_conv_wgrad_workspace_bytes(*args) == 0 and lib.cnl_conv_wgrad_terms(*args) == 0
    assert lib.cnl_relu_grad_workspace_bytes(1, 0, 4, 4) == 0 and lib.cnl_relu_grad_terms(0, 1, 1, 1) == 0
    # the C1 head shape: 64 slices of 64 rows fill the chip; three slices with a short last one; a map smaller than a slice
    assert G.wgrad_geometry(32, 128, 128, 256, 256, 3)["slices"] == 64
    assert (G.wgrad_geometry(2, 9, 64, 32, 1, 3)["slices"], G.wgrad_geometry(2, 9, 64, 32, 1, 3)["rows_per_slice"]) == (3, 8)
    assert G.wgrad_geometry(3, 5, 19, 32, 1, 3)["slices"] == 1


def rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("case", G.CASES, ids=[",".join(map(str, c)) for c in G.CASES])
def test_restatement_equals_torch_float64_autograd(case):
    N, H, W, Cin, Cout, K = case
    x32, dy32, w32 = G.case_tensors(case)
    rng = np.random.default_rng(7)
    b = rng.standard_normal(Cout)
    x = torch.tensor(x32, dtype=torch.float64, requires_grad=True)
    w = torch.tensor(w32.transpose(0, 3, 1, 2).copy(), dtype=torch.float64, requires_grad=True)          # OIHW
    bias = torch.tensor(b, requires_grad=True)
    dy = torch.tensor(dy32, dtype=torch.float64)
    y = torch.relu(F.conv2d(x, w, bias, padding=K // 2))
    y.backward(dy)
    y64 = G.conv(x32, w32, b, relu=True)
    assert rel(y64, y.detach().numpy()) <= 1e-12
    dz, db = G.relu_grad(dy32, y.detach().numpy())
    assert rel(db, bias.grad.numpy()) <= 1e-12
    assert rel(G.wgrad(x32, dz, K), w.grad.numpy().transpose(0, 2, 3, 1)) <= 1e-12
    assert rel(G.dgrad(dz, w32), x.grad.numpy()) <= 1e-12
    # without the activation: the mask is a copy
    dz0, db0 = G.relu_grad(dy32, None)
    assert np.array_equal(dz0, dy32.astype(np.float64)) and rel(db0, dy32.astype(np.float64).sum(axis=(0, 2, 3))) <= 1e-12


@pytest.mark.parametrize("case", [c for c in G.CASES if c[5] == 3], ids=[",".join(map(str, c)) for c in G.CASES if c[5] == 3])
def test_fold_gradients_equal_torch_through_eval_batchnorm(case):
    N, H, W, Cin, Cout, K = case
    x32, dy32, w32 = G.case_tensors(case)
    rng = np.random.default_rng(11)
    conv = torch.nn.Conv2d(Cin, Cout, K, padding=1, bias=False).double()
    bn = torch.nn.BatchNorm2d(Cout).double().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.tensor(w32.transpose(0, 3, 1, 2).copy()))
        bn.weight.copy_(torch.tensor(rng.uniform(0.5, 1.5, Cout)))
        bn.bias.copy_(torch.tensor(rng.standard_normal(Cout)))
        bn.running_mean.copy_(torch.tensor(rng.standard_normal(Cout)))
        bn.running_var.copy_(torch.tensor(rng.uniform(0.5, 2.0, Cout)))
    x = torch.tensor(x32, dtype=torch.float64)
    y = torch.relu(bn(conv(x)))
    y.backward(torch.tensor(dy32, dtype=torch.float64))
    stats = (bn.running_mean.numpy(), bn.running_var.numpy(), bn.eps)
    wf, bf = G.fold(conv.weight.detach().numpy(), bn.weight.detach().numpy(), bn.bias.detach().numpy(), *stats)
    assert rel(G.conv(x32, wf, bf, relu=True), y.detach().numpy()) <= 1e-12
    dz, db = G.relu_grad(dy32, y.detach().numpy())
    dweight, dgamma, dbeta = G.fold_grad(G.wgrad(x32, dz, K), db, conv.weight.detach().numpy(), bn.weight.detach().numpy(), *stats)
    assert rel(dweight, conv.weight.grad.numpy()) <= 1e-12
    assert rel(dgamma, bn.weight.grad.numpy()) <= 1e-12
    assert rel(dbeta, bn.bias.grad.numpy()) <= 1e-12


def test_dbias_in_the_kernels_order_is_within_its_bound_of_the_float64_sum():
    for C, P in ((1, 700), (3, 257), (80, 513), (300, 300)):
        rng = np.random.default_rng(C)
        dz = (rng.standard_normal((1, C, 1, P)) * np.exp(rng.uniform(-6, 2, (1, C, 1, P)))).astype(np.float32)
        got = G.dbias_as_the_kernel_sums(dz, C).astype(np.float64)
        exact = dz.astype(np.float64).sum(axis=(0, 2, 3))
        assert (np.abs(got - exact) <= (G.RG_PIX + 1 + 2) * G.U * np.abs(dz.astype(np.float64)).sum(axis=(0, 2, 3))).all()


def test_cpu_tensors_raise():
    import centernet_lightning_amd as cl
    with pytest.raises(RuntimeError, match="HIP device"):
        cl.conv2d_nhwc(torch.zeros(1, 32, 4, 4), torch.zeros(4, 3, 3, 32), None)
