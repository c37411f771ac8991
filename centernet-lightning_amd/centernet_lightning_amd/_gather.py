"""The one host path into the gather launch (csrc/letterbox.hip) that letterbox_uint8, tile_uint8, letterbox_yuv420 and tile_yuv420
share: records -> one pinned upload -> one launch.  No device sync anywhere.  crop_detections and draw_detections build their
whole-frame records with the same packer (pack_records) and upload them the same way (upload).  The windows and the (plain, planes)
records come from a frame source (_frames.Frames.records)."""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib


def require_hip(tensors, what: str) -> None:
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{what} runs on HIP devices only (no CPU fallback)")


class Gathered(NamedTuple):
    """What gather returns: the canvas and views of the one uploaded device buffer (None for the parts that were not asked for)."""
    canvas: torch.Tensor                         # [V, height, width, C] uint8
    table: torch.Tensor                          # [V, 5] int64: cnl_letterbox_frame records
    yuv_table: Optional[torch.Tensor]            # [V, 9] int64: cnl_yuv420_frame records
    merge_table: Optional[torch.Tensor]          # [V, 8] int32: the merge's view records
    first_view: Optional[torch.Tensor]           # [N + 1] int32


def pack_plain(rec, windows, plain) -> None:
    """Fill rec ([V, 5] int64, zeroed) with the cnl_letterbox_frame records (8-byte pointer + 8 int32) of the V windows
    [(frame, y0, x0, h, w, new_h, new_w, pad_top, pad_left)]; plain[i] = (address, row stride) of window i."""
    import numpy as np
    assert ctypes.sizeof(_lib.LetterboxFrame) == 40
    V = len(windows)
    rec[:, 0] = [address for (address, _) in plain]
    rec.view(np.int32).reshape(V, 10)[:, 2:9] = [(h, w, stride, nh, nw, pt, pl)
                                                 for (_, _, _, h, w, nh, nw, pt, pl), (_, stride) in zip(windows, plain)]


def pack_yuv(rec, windows, planes) -> None:
    """Fill rec ([V, 9] int64, zeroed) with the cnl_yuv420_frame records (3 pointers + 12 int32) of the V windows;
    planes[i] = (y, u, v addresses, y_pitch, c_pitch, c_step) of window i."""
    import numpy as np
    assert ctypes.sizeof(_lib.Yuv420Frame) == 72
    V = len(windows)
    rec[:, :3] = [p[:3] for p in planes]
    rec.view(np.int32).reshape(V, 18)[:, 6:17] = [tuple(p[3:]) + (x0, y0, h, w, nh, nw, pt, pl)
                                                  for p, (_, y0, x0, h, w, nh, nw, pt, pl) in zip(planes, windows)]


def pack_records(windows, plain, planes=None, tail_words: int = 0):
    """-> the zeroed int64 numpy buffer [V x 9] cnl_yuv420_frame records (planes given) or [V x 5] cnl_letterbox_frame records, then
    tail_words words for the caller.  windows, plain, planes: as Frames.records gives them.  Needs neither a device nor the library."""
    import numpy as np
    V, words = len(windows), 9 if planes is not None else 5
    buf = np.zeros(V * words + tail_words, dtype=np.int64)
    if planes is not None:
        pack_yuv(buf[:V * 9].reshape(V, 9), windows, planes)
    else:
        pack_plain(buf[:V * 5].reshape(V, 5), windows, plain)
    return buf


def upload(buf, dev) -> torch.Tensor:
    """The int64 numpy buffer -> device memory through one pinned staging tensor, asynchronously (call under torch.cuda.device(dev))."""
    host = torch.empty((buf.size,), dtype=torch.int64, pin_memory=True)
    host.copy_(torch.from_numpy(buf))
    return host.to(dev, non_blocking=True)


def upload_parts(parts, dev):
    """numpy arrays (int64 / float64 / int32 / float32) -> device tensors of the same dtype and shape, through ONE pinned staging buffer and
    one asynchronous copy (call under torch.cuda.device(dev))."""
    import numpy as np
    words = [-(-p.nbytes // 8) for p in parts]
    buf = np.zeros((max(sum(words), 1),), dtype=np.int64)
    at = 0
    for p, w in zip(parts, words):
        buf[at:at + w].view(np.uint8)[:p.nbytes] = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
        at += w
    dev_buf = upload(buf, dev)
    out, at = [], 0
    for p, w in zip(parts, words):
        out.append(dev_buf[at:at + w].view(getattr(torch, p.dtype.name))[:p.size].view(p.shape))
        at += w
    return out


def gather(dev, windows, plain, height: int, width: int, C: int, word: int, planes=None, coef=None, merge_records=None,
           frame_first_view=None) -> Gathered:
    """One pinned upload and one launch for the V windows [(frame, y0, x0, h, w, new_h, new_w, pad_top, pad_left)].

    plain[i] = (address, row stride) of window i as a packed frame: its cnl_letterbox_frame record, which the launch reads unless
    `planes` is given and unletterbox reads in any case.  planes[i] = (y, u, v addresses, y_pitch, c_pitch, c_step) of window i with
    the six integers `coef`: the cnl_yuv420_frame records, and cnl_letterbox_yuv420_u8 is the launch.  merge_records ([V x 8] int32
    words) and frame_first_view (N + 1 entries): the tables of a tiled gather.  The buffer is [V x 9] int64 YUV records | [V x 5] int64
    plain records | [V x 4] int64 merge records | N + 1 int32 (padded to int64), absent parts left out."""
    import numpy as np
    V = len(windows)
    n_first = len(frame_first_view) if merge_records is not None else 0
    o_plain = V * 9 if planes is not None else 0
    o_merge = o_plain + V * 5
    o_first = o_merge + (V * 4 if merge_records is not None else 0)
    # pack_records writes the records the launch reads, which come first ([V x 9] YUV or [V x 5] plain), and leaves the rest of the
    # layout above as its zeroed tail: [lead records | tail]; of a YUV gather the tail starts with the plain records.
    lead = o_plain if planes is not None else o_merge
    buf = pack_records(windows, plain, planes, tail_words=o_first + (n_first + 1) // 2 - lead)
    assert ctypes.sizeof(_lib.MergeView) == 32
    if planes is not None:                       # the launch reads the YUV records; unletterbox reads the plain ones
        pack_plain(buf[o_plain:o_merge].reshape(V, 5), windows, plain)
    if merge_records is not None:
        buf[o_merge:o_first].view(np.int32).reshape(V, 8)[:] = np.array(merge_records, dtype=np.int32)
        buf[o_first:].view(np.int32)[:n_first] = frame_first_view
    lib = _lib.load()
    with torch.cuda.device(dev):
        d = upload(buf, dev)
        out = Gathered(canvas=torch.empty((V, height, width, C), device=dev, dtype=torch.uint8),
                       table=d[o_plain:o_merge].view(V, 5),
                       yuv_table=d[:o_plain].view(V, 9) if planes is not None else None,
                       merge_table=d[o_merge:o_first].view(torch.int32).view(V, 8) if merge_records is not None else None,
                       first_view=d[o_first:].view(torch.int32)[:n_first] if merge_records is not None else None)
        stream = _lib.stream(dev)
        # the two entry points differ in one argument: the six colour integers where the packed one takes C
        entry, table, c = (("cnl_letterbox_yuv420_u8", out.yuv_table, (ctypes.c_int32 * 6)(*coef)) if planes is not None else
                           ("cnl_letterbox_bilinear_u8", out.table, C))
        _lib.check(getattr(lib, entry)(table.data_ptr(), out.canvas.data_ptr(), V, height, width, c, word, stream), entry)
    return out
