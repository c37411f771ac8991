"""The one reader of per-image targets, for detection_loss, reid_loss, augment_batch / warp_batch and CocoEvaluator.update (its list of
predictions too).  Targets come in two forms: the reference's list of per-image dicts {"boxes" [n, 4], column [n], ...}, which read_list
checks and zero-pads on the host, and the padded form {"boxes" [N, G, 4], column [N, G], ..., "count" [N] int32} of device tensors (a dict, or
a tuple in the order of TUPLE), which read_padded checks and uses in place.  A consumer states its columns once (columns()), and per call
which of them are optional, its cap on G and the tuple lengths it takes; the wording of every complaint is here, once.  A malformed call is a
ValueError wherever its tensors live; a CPU tensor in a well-formed call is the "HIP devices only" RuntimeError."""
import collections

import numpy as np
import torch

from . import _gather

TUPLE = ("boxes", "labels", "count", "ids")      # the padded form as a tuple, by position: its first three or all four
Column = collections.namedtuple("Column", "name numpy torch rank")        # its two dtypes and the dimensions of its padded tensor


def columns(*named, boxes="float64"):
    """("labels", "int64"), ... -> the spec both readers take: the Column of the boxes, of the named columns in order, and of the count."""
    return tuple(Column(name, np.dtype(t), getattr(torch, t), rank) for name, t, rank in (("boxes", boxes, 3), *((n, t, 2) for n, t in named), ("count", "int32", 1)))


LABELS, IDS = columns(("labels", "int64")), columns(("ids", "int64"))


def is_padded(targets, lengths=(3,)):
    """Is this the padded form: a dict, or a tuple / list of tensors whose length is one of `lengths`?"""
    return isinstance(targets, dict) or (isinstance(targets, (list, tuple)) and len(targets) in lengths and
                                         all(isinstance(t, torch.Tensor) for t in targets))


def read_list(items, N, spec, what, arg="targets", against="outputs", optional=(), cap=None, row_ok=None, cannot=None):
    """items: N per-image dicts (N None: as many as there are) of "boxes" [n, 4] and the columns [n] of `spec`, as lists, numpy or tensors.  A
    column named in `optional` is in every image or in none.  At most `cap` boxes per image; row_ok(boxes [n, 4], first column [n]) -> the
    mask of the rows the consumer can take (asked once, for the rows of all images), any other row raising with cannot(its first column's value).
    -> ({"boxes" [N, Gmax, 4], column [N, Gmax] (None for an absent optional one), "count" [N] int32}, Gmax) as zero-padded numpy of the
    spec's dtypes, Gmax = max(1, the most boxes of an image)."""
    if not isinstance(items, (list, tuple)):
        raise ValueError(f"{what}: {arg} must be a list of per-image dicts or padded device tensors, got {type(items).__name__}")
    if N is not None and len(items) != N:
        raise ValueError(f"{what}: {N} images of {against} against {len(items)} of {arg}")
    N, absent = len(items), []
    for name in optional:
        has = [isinstance(d, dict) and name in d for d in items]
        if any(has) and not all(has):
            raise ValueError(f"{what}: either every one of {arg} has '{name}' or none has")
        if not any(has):
            absent.append(name)
    spec = [c for c in spec if c.name != "count" and c.name not in absent]
    keys, pairs, rest = [c.name for c in spec], [(c.name, c.numpy) for c in spec], range(1, len(spec))
    images, sizes = [], []
    for i, d in enumerate(items):
        if not isinstance(d, dict):
            raise ValueError(f"{what}: {arg}[{i}] must be a dict with {', '.join(repr(k) for k in keys)}")
        row = []
        try:
            for k, t in pairs:
                a = d[k]
                if isinstance(a, torch.Tensor):
                    a = a.detach().cpu().numpy()
                a = np.asarray(a)
                row.append(a if a.dtype == t else a.astype(t))
        except KeyError:
            raise ValueError(f"{what}: {arg}[{i}] must be a dict with {', '.join(repr(k) for k in keys)}") from None
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: {arg}[{i}] is not numeric: {e}") from e
        b = row[0]
        if b.size == 0:
            b = row[0] = b.reshape(0, 4)
        fits = b.ndim == 2 and b.shape[1] == 4
        for j in rest:
            c = row[j]
            if c.ndim != 1:
                c = row[j] = c.reshape(-1)
            fits = fits and c.shape[0] == b.shape[0]
        if not fits:
            raise ValueError(f"{what}: {arg}[{i}] has boxes {b.shape} against {', '.join(f'{k} {c.shape}' for k, c in zip(keys[1:], row[1:]))}; "
                             "expected [n, 4] and [n]")
        if cap is not None and b.shape[0] > cap:
            raise ValueError(f"{what}: {arg}[{i}] has {b.shape[0]} boxes; at most {cap} per image are supported")
        images.append(row)
        sizes.append(b.shape[0])
    count = np.array(sizes, dtype=np.int32)
    Gmax = max(sizes + [1])
    out = {name: None for name in absent}
    out.update({c.name: np.zeros((N, Gmax, 4)[:c.rank], dtype=c.numpy) for c in spec})
    if N:
        rows = [np.concatenate([row[j] for row in images]) for j in range(len(spec))]          # all images' rows, image after image
        if row_ok is not None:
            bad = np.nonzero(~row_ok(rows[0], rows[1]))[0]
            if bad.size:
                r = int(bad[0])
                i = int(np.searchsorted(np.cumsum(count), r, side="right"))
                raise ValueError(f"{what}: {arg}[{i}] box {r - sum(sizes[:i])} = {rows[0][r].tolist()} {cannot(int(rows[1][r]))}")
        live = np.arange(Gmax) < count[:, None]
        for c, flat in zip(spec, rows):
            out[c.name][live] = flat
    out["count"] = count
    return out, Gmax


def _shape(N, dim, rank):
    return "[" + ",".join((str(N), dim, "4")[:rank]) + "]"


def _refuse_form(targets, spec, what, arg, dim, optional):
    """The complaint about a padded form with a key, a type, a dtype or a rank out of order: the first of them, keys before tensors."""
    for c in spec:
        if c.name not in targets and c.name not in optional:
            raise ValueError(f"{what}: device {arg} need " + ", ".join(f"'{c.name}' {_shape('N', dim, c.rank)} {c.numpy}" for c in spec if c.name not in optional))
    for c in spec:
        v = targets.get(c.name)
        if not isinstance(v, torch.Tensor):
            if v is None and c.name in optional:
                continue
            raise ValueError(f"{what}: {arg} '{c.name}' must be a tensor, got {type(v).__name__}")
        if v.dtype != c.torch or v.dim() != c.rank:
            raise ValueError(f"{what}: {arg} '{c.name}' must be {c.torch} with {c.rank} dimensions, got {v.dtype} {tuple(v.shape)}")


def read_padded(targets, N, spec, what, arg="targets", one="target", dim="Gmax", optional=(), cap=None, device=None):
    """targets: the padded form, a dict, or a tuple whose positions TUPLE names (one that is no column is not read; the caller has told the
    lengths it takes apart with is_padded), with N images (N None: as many as the boxes have) and 1 <= G <= cap slots per image.  A column or
    the count named in `optional` may be absent or None.  `device`: where the tensors must live (None: all on the device of the boxes).  `arg`,
    `one` and `dim` are the messages' words for the argument, one of its entries and G.
    -> ({name: contiguous device tensor, or None}, G, the device)"""
    if not isinstance(targets, dict):
        targets = dict(zip(TUPLE, targets))
    live = []
    for k, _, dtype, rank in spec:
        v = targets.get(k)
        if v is None and k in optional:
            continue
        if not isinstance(v, torch.Tensor) or v.dtype != dtype or v.dim() != rank:
            _refuse_form(targets, spec, what, arg, dim, optional)
        live.append((k, v, rank))
    boxes = live[0][1]
    G = boxes.shape[1]
    full = (boxes.shape[0] if N is None else N, G, 4)
    for _, v, rank in live:
        if v.shape != full[:rank]:
            raise ValueError(f"{what}: expected {one} {', '.join(f'{k} {_shape(full[0], dim, r)}' for k, _, r in live)}, got "
                             f"{', '.join(str(tuple(v.shape)) for _, v, _ in live)}")
    if G < 1 or (cap is not None and G > cap):
        raise ValueError(f"{what}: {dim} = {G} per image; {'at least 1 is' if cap is None else f'1..{cap} are'} supported")
    if device is None:
        device = boxes.device
    out = dict.fromkeys(optional)
    for k, v, _ in live:
        if not v.is_cuda:
            _gather.require_hip([v], what)
        if v.device != device:
            raise ValueError(f"{what}: {arg} '{k}' lives on {v.device}, expected {device}")
        out[k] = v.contiguous()
    return out, G, device
