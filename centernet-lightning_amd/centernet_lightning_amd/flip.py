"""The flip test (test-time augmentation of the original CenterNet) on the GPU: the network also sees every image mirrored left-right,
and the two sets of head outputs are averaged before pseudo-NMS and top-k.

    doubled = mirror_append_uint8(canvas)               # [2N,H,W,3]: the images, then the images mirrored (cnl_mirror_append_u8)
    merged = flip_merge(model.forward_uint8(doubled), N)  # one launch for all head maps (cnl_flip_merge_f32)

CenterNet.forward / get_encoded_outputs / forward_uint8 / detect_frames / detect_tiled do both behind flip_test=True.

The rule (include/centernet_gfx950.h, restated in torch by tests/flip_ref.py): input N + n is input n mirrored at the network input; the
input width is a multiple of 32 and the stride divides it, so input column x is feature column W - 1 - x exactly, and

    merged[n, c, y, x] = 0.5 * (out[n, c, y, x] + out[N + n, p(c), y, W - 1 - x])

with p(c) = c, except that box_2d (left, top, right, bottom) swaps its channels 0 and 2.  One fp32 add and one multiply by 0.5: equal to
(a + b.flip(-1)[:, perm]) * 0.5 in torch bit for bit.  box_2d is averaged as the raw head output, before the decode's exp / multiplier /
clamp: with box_log that is an average of logarithms, i.e. a geometric mean of the box sizes.
"""
import torch

from . import _lib

SWAP_LR = ("box_2d",)          # the maps whose channels 0 and 2 trade places under a mirror
_HIP_ONLY = "the flip test runs on HIP devices only: move the tensors to 'cuda' (no CPU fallback)"


def mirror_append_uint8(canvas: torch.Tensor) -> torch.Tensor:
    """uint8 frames [N,H,W,C] (C in 1..4) on the GPU -> [2N,H,W,C]: out[n] = canvas[n], out[N + n, y, x] = canvas[n, y, W - 1 - x].
    One launch of cnl_mirror_append_u8."""
    if not isinstance(canvas, torch.Tensor):
        raise TypeError(f"canvas must be a torch.Tensor, got {type(canvas).__name__}")
    if canvas.dtype != torch.uint8 or canvas.dim() != 4 or not 1 <= canvas.shape[-1] <= 4:
        raise ValueError(f"expected uint8 frames [N,H,W,C] with C in 1..4, got {canvas.dtype} {tuple(canvas.shape)}")
    if not canvas.is_cuda:
        raise RuntimeError(_HIP_ONLY)
    canvas = canvas.contiguous()
    N, H, W, C = canvas.shape
    lib = _lib.load()
    with torch.cuda.device(canvas.device):
        # The doubled batch is ONE tensor, for ONE forward: both halves then come from the same plan and launch list whatever N is (two
        # forwards of N would also pay every launch of the plan twice at half the work).  Nothing forces it: a plan's head outputs are
        # fresh tensors per call (engine.Plan.run), only its intermediate activations live in the plan's arena.
        out = torch.empty((2 * N, H, W, C), device=canvas.device, dtype=torch.uint8)
        _lib.check(lib.cnl_mirror_append_u8(canvas.data_ptr(), out.data_ptr(), N, H, W, C, _lib.stream(canvas.device)), "cnl_mirror_append_u8")
    return out


def mirror_append(x: torch.Tensor) -> torch.Tensor:
    """The doubled input of forward(x, flip_test=True) for a float batch [N,3,H,W]: torch.cat((x, x.flip(-1))).  (The video path is
    uint8: mirror_append_uint8.)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise RuntimeError(_HIP_ONLY)
    if x.dim() != 4:
        raise ValueError(f"expected input of shape [N,3,H,W], got {tuple(x.shape)}")
    return torch.cat((x, x.flip(-1)))


def flip_merge(outputs, N: int):
    """outputs: the dict or namedtuple of a forward of 2N inputs (mirror_append_uint8 / mirror_append), every map logical [2N,C,H,W]
    float32 with any strides -> the same type for N images.  Each merged map is a dense [N,H,W,C] allocation returned as the
    logical-NCHW view the engine's own outputs have (the decode keeps its channels-last path).  "box_2d" swaps its channels 0 and 2.
    One launch of cnl_flip_merge_f32 per three maps; no sync."""
    if isinstance(outputs, dict):
        names, maps = list(outputs.keys()), list(outputs.values())
    elif isinstance(outputs, tuple) and hasattr(outputs, "_fields"):
        names, maps = list(outputs._fields), list(outputs)
    else:
        raise TypeError(f"outputs must be the dict or namedtuple of a forward, got {type(outputs).__name__}")
    if isinstance(N, bool) or not isinstance(N, int) or N < 0:
        raise ValueError(f"N must be a non-negative int, got {N!r}")
    if not maps:
        raise ValueError("flip_merge: no maps")
    for name, t in zip(names, maps):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"{name}: expected float32 [2N,C,H,W], got {t.dtype} {tuple(t.shape)}")
        if t.shape[0] != 2 * N:
            raise ValueError(f"{name}: a flip-test forward of {N} images has {2 * N} outputs (the images, then their mirrors), got {t.shape[0]}")
        if tuple(t.shape[2:]) != tuple(maps[0].shape[2:]):
            raise ValueError(f"{name}: map size {tuple(t.shape[2:])} differs from {names[0]}'s {tuple(maps[0].shape[2:])}")
        if name in SWAP_LR and t.shape[1] != 4:
            raise ValueError(f"{name}: expected 4 channels (left, top, right, bottom), got {t.shape[1]}")
    if not all(t.is_cuda for t in maps):
        raise RuntimeError(_HIP_ONLY)
    dev = maps[0].device
    if any(t.device != dev for t in maps):
        raise ValueError("flip_merge: the maps live on different devices")
    H, W = maps[0].shape[2:]
    lib = _lib.load()
    merged = []
    with torch.cuda.device(dev):
        for i in range(0, len(maps), 3):
            group = maps[i:i + 3]
            table = (_lib.FlipMap * len(group))()
            for rec, name, t in zip(table, names[i:i + 3], group):
                C = t.shape[1]
                out = torch.empty((N, H, W, C), device=dev, dtype=torch.float32).permute(0, 3, 1, 2)
                sn, sc, sh, sw = t.stride()
                rec.a, rec.b, rec.dst = t.data_ptr(), t.data_ptr() + 4 * N * sn, out.data_ptr()
                rec.a_sn, rec.a_sc, rec.a_sh, rec.a_sw = rec.b_sn, rec.b_sc, rec.b_sh, rec.b_sw = sn, sc, sh, sw
                rec.d_sn, rec.d_sc, rec.d_sh, rec.d_sw = out.stride()
                rec.C, rec.swap_lr = C, int(name in SWAP_LR)
                merged.append(out)
            _lib.check(lib.cnl_flip_merge_f32(table, len(group), N, H, W, _lib.stream(dev)), "cnl_flip_merge_f32")
    if isinstance(outputs, dict):
        return type(outputs)(zip(names, merged))
    return type(outputs)(*merged)
