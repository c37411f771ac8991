"""The flip-test rule of include/centernet_gfx950.h (cnl_flip_merge_f32, cnl_mirror_append_u8) restated in torch on the CPU.

For a batch of N images the network ran on 2N inputs, input N + n being input n mirrored left-right.  For a head map [2N, C, H, W]:

    merged[n, c, y, x] = 0.5f * (out[n, c, y, x] + out[N + n, p(c), y, W - 1 - x])

p(c) = c, except for the box map (left, top, right, bottom), where channels 0 and 2 trade places.  One IEEE fp32 add, one multiply by
0.5: every comparison against this file is an equality of bit patterns."""
import numpy as np
import torch

SWAP_LR = ("box_2d",)


def perm(C, swap_lr):
    p = list(range(C))
    if swap_lr:
        assert C == 4, "a box map has 4 channels"
        p[0], p[2] = 2, 0
    return p


def merge(maps_2n, swap_lr=False):
    """maps_2n: float32 [2N, C, H, W] (tensor or array, any device) -> merged [N, C, H, W] float32 on the CPU."""
    t = torch.as_tensor(maps_2n).detach().cpu().contiguous()
    assert t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] % 2 == 0, (t.dtype, tuple(t.shape))
    N = t.shape[0] // 2
    a, b = t[:N], t[N:]
    return (a + b.flip(-1)[:, perm(t.shape[1], swap_lr)]) * 0.5


def merge_outputs(outputs):
    """The dict or namedtuple of a 2N forward -> a dict name -> merged CPU tensor ("box_2d" swaps)."""
    items = outputs.items() if isinstance(outputs, dict) else zip(outputs._fields, outputs)
    return {name: merge(t, name in SWAP_LR) for name, t in items}


def mirror_append(u8):
    """uint8 [N, H, W, C] -> [2N, H, W, C] on the CPU: the images, then the images with their columns reversed."""
    t = torch.as_tensor(u8).detach().cpu()
    assert t.dtype == torch.uint8 and t.dim() == 4, (t.dtype, tuple(t.shape))
    return torch.cat((t, t.flip(2))).contiguous()


def mirror_maps(merged):
    """The mirror image of merged maps {name: [N, C, H, W]}: columns reversed, box channels 0 and 2 swapped."""
    return {name: torch.as_tensor(t).detach().cpu().flip(-1)[:, perm(t.shape[1], name in SWAP_LR)].contiguous() for name, t in merged.items()}


def same_bits(got, want):
    """NaN positions match and every other element has the same bit pattern."""
    g, w = torch.as_tensor(got).detach().cpu().contiguous(), torch.as_tensor(want).detach().cpu().contiguous()
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype != torch.float32:
        return torch.equal(g, w)
    gn, wn = torch.isnan(g), torch.isnan(w)
    return torch.equal(gn, wn) and np.array_equal(g.numpy().view(np.uint32)[~gn.numpy()], w.numpy().view(np.uint32)[~wn.numpy()])
