"""ORACLE — TEST INFRASTRUCTURE ONLY.  Seeded synthetic-input recipes shared by oracle/make_golden.py
(build container) and the tests/bench (GPU box), so large golden cases store only
{recipe name, seed, shape, SHA-256 of the input bytes} + the reference's outputs.

Conventions follow SURVEY.md §8(d) / BASELINE.md §5: heat = sigmoid(randn - 2.19) (init_bias of
configs/base_resnet34.yaml:16), box = rand * 16, reid = randn; images = rand in [0,1]
(tests/test_models.py:12 of the reference).
"""
import hashlib

import numpy as np
import torch

import ref_cpu


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def decode_inputs(seed, shape, emb_dim=0):
    """-> heat (N,C,H,W) f32 in (0,1), box (N,4,H,W) f32 in [0,16) [, reid (N,E,H,W)] as torch CPU."""
    N, C, H, W = shape
    g = _gen(seed)
    heat = torch.randn(N, C, H, W, generator=g).sub_(2.19).sigmoid_()
    box = torch.rand(N, 4, H, W, generator=g).mul_(16.0)
    out = [heat, box]
    if emb_dim:
        out.append(torch.randn(N, emb_dim, H, W, generator=g))
    return out


def images(seed, shape):
    return torch.rand(*shape, generator=_gen(seed))


def sha256(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
        h.update(a.tobytes())
    return h.hexdigest()


def _trained_checkpoint_like(sd):
    """BatchNorm scales as a trained checkpoint has them: every BN gamma times 10^U(-2, 0.5) per channel, 5 % of the channels dead
    (gamma = beta = 0: the folded filter and its bias are exactly zero) — the FOLDED conv weights then spread over 2.5 decades per output
    channel and so do the activations the next layer reads; running statistics re-calibrated so that the network stays O(1)."""
    g = torch.Generator().manual_seed(77)
    for k in list(sd):
        if k.endswith("running_var"):
            base = k[: -len("running_var")]
            c = sd[k].numel()
            s = torch.pow(10.0, torch.rand(c, generator=g) * 2.5 - 2.0)
            s[torch.randperm(c, generator=g)[: max(1, c // 20)]] = 0.0
            sd[base + "weight"].mul_(s)
            sd[base + "bias"].mul_((s > 0).float())
    ref_cpu.forward(sd, torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(99)) * 4.2 - 2.1, stats=True)
