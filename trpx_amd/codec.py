"""Device-resident entry points: torch tensors in HBM -> trpx_encode / trpx_decode.

torch is plumbing only (device memory + streams); all compute happens in libtrpx_hip.so.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib

_TORCH2DT = {torch.uint8: _lib.U8, torch.int8: _lib.I8, torch.uint16: _lib.U16, torch.int16: _lib.I16,
             torch.uint32: _lib.U32, torch.int32: _lib.I32, torch.uint64: _lib.U64, torch.int64: _lib.I64}
_NP2TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int8): torch.int8, np.dtype(np.uint16): torch.uint16,
             np.dtype(np.int16): torch.int16, np.dtype(np.uint32): torch.uint32, np.dtype(np.int32): torch.int32,
             np.dtype(np.uint64): torch.uint64, np.dtype(np.int64): torch.int64}
BLOCK = 12


def dtype_code(dt) -> int:
    if isinstance(dt, torch.dtype):
        return _TORCH2DT[dt]
    return _TORCH2DT[_NP2TORCH[np.dtype(dt)]]


def torch_dtype(dt) -> torch.dtype:
    return dt if isinstance(dt, torch.dtype) else _NP2TORCH[np.dtype(dt)]


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: torch.Tensor | None):
    return t.data_ptr() if t is not None else None


def _status(status: torch.Tensor | None, dev) -> torch.Tensor:
    return status if status is not None else torch.empty(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)


def worst_case_bytes(dtype, n_values: int, block: int = BLOCK) -> int:
    return lib().trpx_worst_case_bytes(dtype_code(dtype), n_values, block)


@dataclass
class Encoded:
    """A compact TERSE stack in HBM (= the reference's d_terse_data, Terse.hpp:482)."""
    data: torch.Tensor           # uint8, capacity sized; the stack is data[:total_bytes]
    frame_offsets: torch.Tensor  # int64 [n_frames + 1], byte offset of every frame, [-1] = total
    status: torch.Tensor         # int32 [8]; [0] error code, [1] prolix_bits
    n_values: int
    n_frames: int
    dtype: torch.dtype
    index: torch.Tensor | None = None   # optional decode index (trpx_encode_indexed)
    _retry: tuple | None = None         # what check() needs to run the call again (see check)

    def total_bytes(self) -> int:
        return int(self.frame_offsets[-1].item())

    def prolix_bits(self) -> int:
        return int(self.status[1].item())

    def check(self) -> None:
        """Synchronises and raises on a device error.  A look-back timeout of the single-pass encoder (TRPX_ERR_TIMEOUT,
        see trpx_encode_checked in include/trpx_hip.h) is not an error of the data: the call is run again through the
        two-pass pipeline (trpx_encode_checked), which writes the identical stream -- from the pixel tensor and workspace
        the encode was given, which this object keeps alive: ``px`` must still hold the encoded frames when ``check()`` runs
        (a caller that recycles its pixel buffer calls ``check()`` first)."""
        code = int(self.status[0].item())
        if code == _lib.ERR_TIMEOUT and self._retry is not None:
            px, ws, block = self._retry
            with torch.cuda.device(px.device):
                check(lib().trpx_encode_checked(dtype_code(px.dtype), px.data_ptr(), self.n_values, self.n_frames, block,
                                                self.data.data_ptr(), self.data.numel(), self.frame_offsets.data_ptr(),
                                                self.status.data_ptr(), _ptr(self.index), ws.data_ptr(), ws.numel(), _stream_ptr(px), None))
            code = int(self.status[0].item())
        if code:
            raise _lib.TrpxError(code, "device status after encode")

    def stack(self) -> torch.Tensor:
        return self.data[: self.total_bytes()]


class Workspace:
    """Caller-owned scratch so that the hot path never allocates."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes:
            self.release()
            self.buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return self.buf

    def release(self) -> None:
        """The buffer goes back to torch's allocator, which may hand its address to anything: the library must forget what it
        remembers about it (trpx_workspace_invalidate: include/trpx_hip.h, "Workspaces between calls")."""
        if self.buf is not None:
            try:
                lib().trpx_workspace_invalidate(self.buf.data_ptr(), self.buf.numel())
            except Exception:          # (interpreter shutdown)
                pass
            self.buf = None

    def __del__(self):
        self.release()


def _scratch(workspace: Workspace | None, dev, nbytes: int) -> torch.Tensor:
    return (workspace or Workspace(dev)).get(nbytes)


def _out(fn: str, out: torch.Tensor | None, shape, dtype, dev, type_name: str | None = None, also=()) -> torch.Tensor:
    """A consumer's output: a new tensor of this shape and dtype on dev, or the caller's checked against them (also: other
    dtypes of the same size it may have; type_name: how the message names the type)."""
    if out is None:
        return torch.empty(tuple(max(s, 0) for s in shape), dtype=dtype, device=dev)   # (a negative count: left to the library)
    if out.dtype not in (dtype, *also) or out.numel() != math.prod(shape) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{fn}: out must be a contiguous {type_name or dtype} tensor of {' x '.join(map(str, shape))} elements on {dev}")
    return out


def _consumer_ws(workspace: Workspace | None, dev, frame_offsets, index, always: bool, name: str, *args) -> torch.Tensor | None:
    """The workspace of a call of the consumer trpx_decode_<name>, as large as its query says for args.  always: the consumer
    has scratch of its own, so every form of the call brings one; otherwise only a form without offsets or index does (None:
    the call needs none)."""
    if always or frame_offsets is None or index is None:
        return _scratch(workspace, dev, getattr(lib(), f"trpx_decode_{name}_workspace_bytes")(*args))
    return None


def _numel(t: torch.Tensor | None) -> int:
    return t.numel() if t is not None else 0


def index_bytes(dtype, n_values: int, n_frames: int, block: int = BLOCK) -> int:
    return lib().trpx_index_bytes(dtype_code(dtype), n_values, n_frames, block)


def encode(pixels: torch.Tensor, out: torch.Tensor | None = None, workspace: Workspace | None = None,
           frame_offsets: torch.Tensor | None = None, status: torch.Tensor | None = None,
           block: int = BLOCK, index: torch.Tensor | bool | None = None) -> Encoded:
    """Encode a [n_frames, n_values] (or [n_frames, H, W]) stack resident on the GPU.

    Asynchronous on the current stream; call ``Encoded.check()`` (synchronises) to test status."""
    if not pixels.is_cuda:
        raise ValueError("pixels must live on the GPU (use trpx_amd.Terse for host data)")
    px = pixels.contiguous()
    n_frames = px.shape[0]
    n_values = px[0].numel()
    code = dtype_code(px.dtype)
    dev = px.device
    if out is None:
        cap = (n_frames * worst_case_bytes(px.dtype, n_values, block) + 15) // 16 * 16
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if frame_offsets is None:
        frame_offsets = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
    status = _status(status, dev)
    ws_bytes = lib().trpx_encode_workspace_bytes(code, n_values, n_frames, block)
    # (no Workspace given: a plain tensor that nobody owns beyond Encoded._retry -- a throw-away Workspace object would
    # invalidate in its destructor BEFORE the call below registers the memory as clean)
    ws = workspace.get(ws_bytes) if workspace is not None else torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    if index is True:     # also keep the decode index (not part of the bitstream)
        index = torch.empty(index_bytes(px.dtype, n_values, n_frames, block), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().trpx_encode_indexed(code, px.data_ptr(), n_values, n_frames, block, out.data_ptr(), out.numel(),
                                        frame_offsets.data_ptr(), status.data_ptr(), _ptr(index), ws.data_ptr(), ws.numel(),
                                        _stream_ptr(px)))
        if workspace is None:
            # The buffer dies with the Encoded object and goes back to torch's allocator, which may hand its address to
            # anything: the library must not remember it as a clean workspace (include/trpx_hip.h, "Workspaces between
            # calls"; the registry is host-side, so forgetting right behind the launch is safe).
            check(lib().trpx_workspace_invalidate(ws.data_ptr(), ws.numel()))
    return Encoded(out, frame_offsets, status, n_values, n_frames, px.dtype, index if index is not None else None, (px, ws, block))


def encode_sparse_workspace_bytes(dtype, n_values: int, n_frames: int, block: int = BLOCK) -> int:
    return lib().trpx_encode_sparse_workspace_bytes(dtype_code(torch_dtype(dtype)), n_values, n_frames, block)


def encode_sparse_bound_bytes(dtype, n_values: int, n_frames: int, n_events: int, block: int = BLOCK) -> int:
    """An upper bound on the stack of ``n_frames`` frames with ``n_events`` events in all (trpx_encode_sparse_bound_bytes)."""
    return lib().trpx_encode_sparse_bound_bytes(dtype_code(torch_dtype(dtype)), n_values, n_frames, n_events, block)


def encode_sparse(row_offsets: torch.Tensor, positions: torch.Tensor | None, values: torch.Tensor | None, n_values: int,
                  n_frames: int, dtype, out: torch.Tensor | None = None, workspace: Workspace | None = None,
                  frame_offsets: torch.Tensor | None = None, status: torch.Tensor | None = None, block: int = BLOCK) -> Encoded:
    """Encode a stack given as its events in CSR form, resident on the GPU (trpx_encode_sparse): frame f is ``n_values`` zeros
    with ``px[f][positions[i]] = values[i]`` for ``row_offsets[f] <= i < row_offsets[f + 1]`` -- what ``decode_sparse`` returns.
    The stream is byte for byte what ``encode`` writes for the dense frames; no decode index is produced (``build_index``).

    ``row_offsets``: int64 or uint64 [n_frames + 1]; ``positions``: uint32 / int32; ``values``: of ``dtype``; both ``None`` for a
    stack of empty frames.  Asynchronous on the current stream; ``Encoded.check()`` (synchronises) raises on status[0]: 1 for
    bad events (a position out of range, a row not strictly ascending, row_offsets decreasing or beyond the lists), 3 when
    ``out`` is too small (``out=None`` allocates ``encode_sparse_bound_bytes``)."""
    tdt = torch_dtype(dtype)
    code = dtype_code(tdt)
    dev = row_offsets.device
    if not row_offsets.is_cuda:
        raise ValueError("encode_sparse: the events must live on the GPU (use trpx_amd.Terse.push_back_sparse for host data)")
    if row_offsets.dtype not in (torch.int64, torch.uint64) or row_offsets.numel() < n_frames + 1 or not row_offsets.is_contiguous():
        raise TypeError(f"encode_sparse: row_offsets must be a contiguous int64 / uint64 tensor of >= {n_frames + 1} elements")
    if (positions is None) != (values is None):
        raise ValueError("encode_sparse: positions and values go together")
    n_events = 0
    if positions is not None:
        n_events = positions.numel()
        if positions.dtype not in (torch.uint32, torch.int32) or values.dtype != tdt or values.numel() != n_events \
                or not positions.is_contiguous() or not values.is_contiguous() or positions.device != dev or values.device != dev:
            raise ValueError(f"encode_sparse: positions (uint32) and values ({tdt}) must be contiguous tensors of one length on {dev}")
    if out is None:
        out = torch.empty(max(encode_sparse_bound_bytes(tdt, n_values, n_frames, n_events, block), 16), dtype=torch.uint8, device=dev)
    if frame_offsets is None:
        frame_offsets = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
    status = _status(status, dev)
    ws = _scratch(workspace, dev, lib().trpx_encode_sparse_workspace_bytes(code, n_values, n_frames, block))
    with torch.cuda.device(dev):
        check(lib().trpx_encode_sparse(code, row_offsets.data_ptr(), positions.data_ptr() if n_events else None,
                                       values.data_ptr() if n_events else None, n_events, n_values, n_frames, block,
                                       out.data_ptr(), out.numel(), frame_offsets.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                       ws.numel(), _stream_ptr(row_offsets)))
    return Encoded(out, frame_offsets, status, n_values, n_frames, tdt)


def decode(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype,
           out: torch.Tensor | None = None, workspace: Workspace | None = None,
           status: torch.Tensor | None = None, stream_signed: bool | None = None,
           block: int = BLOCK, index: torch.Tensor | None = None):
    """Decode a stack resident on the GPU. Returns (pixels [n_frames, n_values], status)."""
    tdt = torch_dtype(dtype)
    code = dtype_code(tdt)
    dev = terse.device
    if stream_signed is None:
        stream_signed = bool(lib().trpx_dtype_is_signed(code))
    if out is None:
        out = torch.empty((n_frames, n_values), dtype=tdt, device=dev)
    status = _status(status, dev)
    if index is not None:   # walk-free decode with a previously kept index
        with torch.cuda.device(dev):
            check(lib().trpx_decode_indexed(int(stream_signed), code, terse.data_ptr(), terse.numel(),
                                            frame_offsets.data_ptr(), index.data_ptr(), n_values, n_frames, block,
                                            out.data_ptr(), status.data_ptr(), _stream_ptr(terse)))
        return out, status
    ws = _scratch(workspace, dev, lib().trpx_decode_workspace_bytes(code, n_values, n_frames, block))
    with torch.cuda.device(dev):
        check(lib().trpx_decode(int(stream_signed), code, terse.data_ptr(), terse.numel(), _ptr(frame_offsets),
                                n_values, n_frames, block, out.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                ws.numel(), _stream_ptr(terse)))
    return out, status


def locate_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, block: int = BLOCK) -> int:
    return lib().trpx_locate_workspace_bytes(terse_bytes, n_values, n_frames, block)


def _max_bits(dtype) -> int:
    return 8 * lib().trpx_dtype_size(dtype_code(torch_dtype(dtype)))


def locate_frames(terse: torch.Tensor, n_values: int, n_frames: int, dtype, block: int = BLOCK,
                  workspace: Workspace | None = None, status: torch.Tensor | None = None,
                  out: torch.Tensor | None = None):
    """Frame offsets of an index-free stack resident on the GPU (trpx_locate_frames).  Returns (offsets int64
    [n_frames + 1], status); asynchronous on the current stream, status[0] != 0: corrupt or truncated stack."""
    dev = terse.device
    if out is None:
        out = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
    status = _status(status, dev)
    ws = _scratch(workspace, dev, locate_workspace_bytes(terse.numel(), n_values, n_frames, block))
    with torch.cuda.device(dev):
        check(lib().trpx_locate_frames(terse.data_ptr(), terse.numel(), n_values, n_frames, block, _max_bits(dtype),
                                       out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(terse)))
    return out, status


def build_index(terse: torch.Tensor, frame_offsets: torch.Tensor, n_values: int, n_frames: int, dtype,
                block: int = BLOCK) -> torch.Tensor:
    """Walk an existing stack once and keep the decode index (trpx_build_index)."""
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    index = torch.empty(index_bytes(dtype, n_values, n_frames, block), dtype=torch.uint8, device=dev)
    status = _status(None, dev)
    with torch.cuda.device(dev):
        check(lib().trpx_build_index(code, terse.data_ptr(), terse.numel(), frame_offsets.data_ptr(), n_values,
                                     n_frames, block, index.data_ptr(), status.data_ptr(), _stream_ptr(terse)))
    return index


def synth(dtype, frame0: int, n_frames: int, n_values: int, device="cuda", seed: int = 20240807) -> torch.Tensor:
    """synth-v1 frames generated on the GPU (identical to the oracle's CPU generator)."""
    tdt = torch_dtype(dtype)
    out = torch.empty((n_frames, n_values), dtype=tdt, device=device)
    with torch.cuda.device(out.device):
        check(lib().trpx_synth_fill(dtype_code(tdt), seed, frame0, n_frames, n_values, out.data_ptr(),
                                    _stream_ptr(out)))
    return out


_SUM_OUT = {torch.int32: _lib.I32, torch.uint32: _lib.U32, torch.int64: _lib.I64, torch.uint64: _lib.U64,
            torch.float32: _lib.F32, torch.float64: _lib.F64}


def decode_sum_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, group: int, block: int = BLOCK) -> int:
    return lib().trpx_decode_sum_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block, group)


def decode_sum(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, group: int,
               out_dtype=torch.int32, index: torch.Tensor | None = None, out: torch.Tensor | None = None,
               workspace: Workspace | None = None, status: torch.Tensor | None = None, block: int = BLOCK):
    """Sums of ``group`` consecutive frames of a stack resident on the GPU (trpx_decode_sum), without decoding it to memory.

    ``dtype`` is the stream's pixel type; ``out_dtype`` one of int32, uint32, int64, uint64, float32, float64.  Returns
    (sums [ceil(n_frames / group), n_values], status); asynchronous on the current stream, like ``decode``.
    ``frame_offsets = None``: the frames are located first; ``index = None``: the decode index is built on the way."""
    odt = torch_dtype(out_dtype)
    if odt not in _SUM_OUT:
        raise TypeError(f"decode_sum: out_dtype {odt} (int32, uint32, int64, uint64, float32, float64)")
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    n_out = -(-n_frames // group) if group > 0 else 0
    if out is None:
        out = torch.empty((n_out, n_values), dtype=odt, device=dev)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "sum", code, terse.numel(), n_values, n_frames, block, group)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_sum(code, _SUM_OUT[odt], terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                    n_values, n_frames, block, group, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream_ptr(terse)))
    return out, status


def decode_roi_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, block: int = BLOCK) -> int:
    return lib().trpx_decode_roi_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block)


def decode_roi(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, width: int,
               boxes: torch.Tensor, box_shape, index: torch.Tensor | None = None, out: torch.Tensor | None = None,
               workspace: Workspace | None = None, status: torch.Tensor | None = None, block: int = BLOCK):
    """Boxes of pixels of a stack resident on the GPU (trpx_decode_roi), without decoding its frames to memory.

    ``dtype`` is the stream's pixel type and the output's; ``width`` the row length of a frame; ``boxes`` a contiguous
    ``[n, 3]`` device tensor of int32 / uint32 rows ``(frame, y0, x0)``; ``box_shape = (box_h, box_w)`` for all of them.
    Returns (out [n, box_h, box_w], status); asynchronous on the current stream, like ``decode``.  status[0] is 1 when a box
    leaves the stack (the other boxes are still right) and 5 for a corrupt stream or index; only the parts of the stack the
    boxes touch are validated.  ``frame_offsets = None``: the frames are located first; ``index = None``: the decode index is
    built on the way (both in ``workspace``)."""
    tdt = torch_dtype(dtype)
    code = dtype_code(tdt)
    dev = terse.device
    if boxes.dtype not in (torch.int32, torch.uint32) or boxes.dim() != 2 or boxes.shape[1] != 3 or not boxes.is_contiguous():
        raise TypeError("decode_roi: boxes must be a contiguous [n, 3] tensor of int32 / uint32")
    if boxes.device != dev:
        raise ValueError("decode_roi: boxes must live on the stack's device")
    box_h, box_w = (int(x) for x in box_shape)
    n_boxes = boxes.shape[0]
    out = _out("decode_roi", out, (n_boxes, box_h, box_w), tdt, dev)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, False, "roi", code, terse.numel(), n_values, n_frames, block)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_roi(code, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                    n_values, n_frames, block, width, boxes.data_ptr(), n_boxes, box_h, box_w, out.data_ptr(),
                                    status.data_ptr(), _ptr(ws), _numel(ws), _stream_ptr(terse)))
    return out, status


def decode_sparse_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, block: int = BLOCK) -> int:
    return lib().trpx_decode_sparse_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block)


def decode_sparse(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, threshold: int,
                  index: torch.Tensor | None = None, capacity: int | None = None, row_offsets: torch.Tensor | None = None,
                  positions: torch.Tensor | None = None, values: torch.Tensor | None = None, workspace: Workspace | None = None,
                  status: torch.Tensor | None = None, block: int = BLOCK):
    """The pixels with value >= ``threshold`` of a stack resident on the GPU (trpx_decode_sparse), in CSR form, without decoding
    its frames to memory.

    ``dtype`` is the stream's pixel type and that of the values.  Returns (row_offsets int64 [n_frames + 1], positions uint32,
    values, status): event i of frame f, row_offsets[f] <= i < row_offsets[f + 1], is pixel positions[i] of that frame and has
    value values[i]; events come by frame and, inside a frame, by ascending pixel index.

    With ``capacity`` given: ONE call, asynchronous on the current stream like ``decode``, into tensors of ``capacity`` elements
    (``positions`` / ``values`` if given, which must hold that many); status[0] is 3 when there are more events than that
    (row_offsets is still complete) and 5 for a corrupt stream or index -- the whole stack is validated.  With
    ``capacity=None`` the call SYNCHRONISES: a sizes-only call, one read of the total, exact-size tensors of its own (``positions`` /
    ``values`` may not be given then: ValueError), a second call.
    ``frame_offsets = None``: the frames are located first; ``index = None``: the decode index is built on the way (both in
    ``workspace``)."""
    tdt = torch_dtype(dtype)
    code = dtype_code(tdt)
    dev = terse.device
    if row_offsets is None:
        row_offsets = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "sparse", code, terse.numel(), n_values, n_frames, block)

    def call(pos, val, cap):
        with torch.cuda.device(dev):
            check(lib().trpx_decode_sparse(code, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                           n_values, n_frames, block, int(threshold), row_offsets.data_ptr(), _ptr(pos),
                                           _ptr(val), cap, status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(terse)))

    if capacity is None:
        if positions is not None or values is not None:
            raise ValueError("decode_sparse: positions / values need a capacity (capacity=None sizes and allocates them itself)")
        call(None, None, 0)
        capacity = int(row_offsets[-1].item())               # (synchronises)
        if int(status[0].item()) not in (_lib.OK, _lib.ERR_CAPACITY):
            empty = torch.empty(0, dtype=torch.uint32, device=dev), torch.empty(0, dtype=tdt, device=dev)
            return row_offsets, empty[0], empty[1], status
    if positions is None:
        positions = torch.empty(capacity, dtype=torch.uint32, device=dev)
    if values is None:
        values = torch.empty(capacity, dtype=tdt, device=dev)
    if positions.dtype not in (torch.uint32, torch.int32) or values.dtype != tdt or positions.numel() < capacity or values.numel() < capacity \
            or not positions.is_contiguous() or not values.is_contiguous() or positions.device != dev or values.device != dev:
        raise ValueError(f"decode_sparse: positions (uint32) and values ({tdt}) must be contiguous tensors of >= {capacity} elements on {dev}")
    call(positions, values, capacity)
    return row_offsets, positions, values, status


def decode_dot_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, n_maps: int, block: int = BLOCK) -> int:
    return lib().trpx_decode_dot_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block, n_maps)


def decode_dot(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, weights: torch.Tensor,
               index: torch.Tensor | None = None, out: torch.Tensor | None = None, workspace: Workspace | None = None,
               status: torch.Tensor | None = None, block: int = BLOCK):
    """Per frame the sums of its pixels weighted by K integer maps (trpx_decode_dot), for a stack resident on the GPU, without
    decoding its frames to memory: a mask gives a virtual detector image, the maps x, y and 1 the centre of mass.

    ``dtype`` is the stream's pixel type; ``weights`` a contiguous int32 tensor ``[K, n_values]`` (or ``[K, H, W]`` with
    ``H * W == n_values``) on the stack's device, 1 <= K <= 16.  Returns (dots int64 [n_frames, K], status): ``dots[f, k] =
    sum_p px[f][p] * weights[k][p]``, exact, modulo 2^64; asynchronous on the current stream, like ``decode``.  status[0] is 5
    for a corrupt stream or index -- the whole stack is validated, whatever the maps.  ``frame_offsets = None``: the frames are
    located first; ``index = None``: the decode index is built on the way (both in ``workspace``)."""
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    if weights.dtype != torch.int32 or weights.dim() < 2 or not weights.is_contiguous() or weights.numel() != weights.shape[0] * n_values:
        raise TypeError(f"decode_dot: weights must be a contiguous int32 tensor [K, {n_values}] (or [K, H, W])")
    if weights.device != dev:
        raise ValueError("decode_dot: weights must live on the stack's device")
    n_maps = weights.shape[0]
    if not 1 <= n_maps <= 16:
        raise ValueError("decode_dot: 1 to 16 maps")
    out = _out("decode_dot", out, (n_frames, n_maps), torch.int64, dev, "int64")
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "dot", code, terse.numel(), n_values, n_frames, block, n_maps)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_dot(code, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                    n_values, n_frames, block, weights.data_ptr(), n_maps, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(terse)))
    return out, status


def decode_bins_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, n_bins: int, block: int = BLOCK) -> int:
    return lib().trpx_decode_bins_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block, n_bins)


def decode_bins(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, labels: torch.Tensor,
                n_bins: int, index: torch.Tensor | None = None, out: torch.Tensor | None = None, workspace: Workspace | None = None,
                status: torch.Tensor | None = None, block: int = BLOCK):
    """Per frame the sums of its pixels over the bins of a label map (trpx_decode_bins), for a stack resident on the GPU,
    without decoding its frames to memory: the radial profile (azimuthal integration) of every frame, ring detectors.

    ``dtype`` is the stream's pixel type; ``labels`` a contiguous uint16 (or int16, read as uint16) tensor ``[n_values]`` (or
    ``[H, W]`` with ``H * W == n_values``) on the stack's device; 1 <= n_bins <= 4096.  A label >= n_bins belongs to no bin
    (mask with 0xFFFF).  Returns (bins int64 [n_frames, n_bins], status): ``bins[f, b] = sum of px[f][p] over labels[p] == b``,
    exact, every element written; asynchronous on the current stream, like ``decode``.  status[0] is 5 for a corrupt stream or
    index -- the whole stack is validated, whatever the map.  ``frame_offsets = None``: the frames are located first; ``index =
    None``: the decode index is built on the way (both in ``workspace``)."""
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    if labels.dtype not in (torch.uint16, torch.int16):
        raise TypeError("decode_bins: labels must be a uint16 (or int16-viewed) tensor")
    if labels.dim() < 1 or not labels.is_contiguous() or labels.numel() != n_values:
        raise ValueError(f"decode_bins: labels must be a contiguous tensor of {n_values} elements ([n_values] or [H, W])")
    if labels.device != dev:
        raise ValueError("decode_bins: labels must live on the stack's device")
    if not 1 <= n_bins <= 4096:
        raise ValueError("decode_bins: 1 to 4096 bins")
    out = _out("decode_bins", out, (n_frames, n_bins), torch.int64, dev, "int64")
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "bins", code, terse.numel(), n_values, n_frames, block, n_bins)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_bins(code, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                     n_values, n_frames, block, labels.data_ptr(), n_bins, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(terse)))
    return out, status


def decode_hist_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, n_bins: int, group: int = 1, block: int = BLOCK) -> int:
    return lib().trpx_decode_hist_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block, group, n_bins)


def decode_hist(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, n_bins: int,
                group: int = 1, lo: int = 0, shift: int = 0, index: torch.Tensor | None = None, out: torch.Tensor | None = None,
                workspace: Workspace | None = None, status: torch.Tensor | None = None, block: int = BLOCK):
    """Per group of ``group`` consecutive frames the histogram of its pixel values (trpx_decode_hist), for a stack resident on
    the GPU, without decoding its frames to memory: ``bin(v) = clamp((v - lo) >> shift, 0, n_bins - 1)``, the first and the last
    bin taking everything below and above.

    ``dtype`` is the stream's pixel type; 1 <= n_bins <= 4096, 0 <= shift <= 32, |lo| <= 2^32, group >= 1 (the last group holds
    what is left; ``group = n_frames``: the stack's histogram).  Returns (hist int64 [ceil(n_frames / group), n_bins], status):
    exact counts, every element written, each row summing to n_values x the group's frames; asynchronous on the current stream,
    like ``decode``.  status[0] is 5 for a corrupt stream or index -- the whole stack is validated, whatever is fetched.
    ``frame_offsets = None``: the frames are located first; ``index = None``: the decode index is built on the way (both in
    ``workspace``)."""
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    if not 1 <= n_bins <= 4096:
        raise ValueError("decode_hist: 1 to 4096 bins")
    if not 0 <= shift <= 32 or abs(lo) > 2**32:
        raise ValueError("decode_hist: 0 <= shift <= 32 and |lo| <= 2^32")
    if group < 1:
        raise ValueError("decode_hist: group >= 1")
    n_groups = -(-n_frames // min(group, n_frames)) if n_frames else 0
    out = _out("decode_hist", out, (n_groups, n_bins), torch.int64, dev, "int64", also=(torch.uint64,))   # (counts < 2^63: the uint64 of the C ABI, as int64)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "hist", code, terse.numel(), n_values, n_frames, block, group, n_bins)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_hist(code, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index), n_values, n_frames, block,
                                     group, lo, shift, n_bins, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(terse)))
    return out, status


def decode_corrected_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, block: int = BLOCK) -> int:
    return lib().trpx_decode_corrected_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block)


def _map(name: str, m: torch.Tensor | None, n_values: int, dev) -> torch.Tensor | None:
    if m is not None and (m.dtype != torch.float32 or m.numel() != n_values or not m.is_contiguous() or m.device != dev):
        raise ValueError(f"decode_corrected: {name} must be a contiguous float32 tensor of {n_values} elements on {dev}")
    return m


def decode_corrected(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype,
                     dark: torch.Tensor | None = None, gain: torch.Tensor | None = None, index: torch.Tensor | None = None,
                     out: torch.Tensor | None = None, workspace: Workspace | None = None, status: torch.Tensor | None = None,
                     block: int = BLOCK):
    """Every frame of a stack resident on the GPU as float32 with the dark reference subtracted and the gain reference
    multiplied in (trpx_decode_corrected): ``out[f, p] = (float32(px[f, p]) - dark[p]) * gain[p]``, three float32 operations in
    this order, each rounded once -- bit for bit ``(px.to(torch.float32) - dark) * gain`` wherever that is not subnormal --
    without the integer stack and the float temporaries of that expression.

    ``dtype`` is the stream's pixel type; ``dark`` / ``gain``: float32 ``[n_values]`` on the stream's device, read when the
    kernel runs (a captured call is replayed with new maps in the same tensors), or None to leave the operation out (both None:
    a plain float32 decode).  Returns (out float32 [n_frames, n_values], status): every element written; asynchronous on the
    current stream, like ``decode``.  status[0] is 5 for a corrupt stream or index.  ``frame_offsets = None``: the frames are
    located first; ``index = None``: the decode index is built on the way (both in ``workspace``)."""
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    dark, gain = _map("dark", dark, n_values, dev), _map("gain", gain, n_values, dev)
    out = _out("decode_corrected", out, (n_frames, n_values), torch.float32, dev, "float32")
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, False, "corrected", code, terse.numel(), n_values, n_frames, block)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_corrected(code, _lib.F32, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index), n_values, n_frames,
                                          block, _ptr(dark), _ptr(gain), out.data_ptr(), status.data_ptr(), _ptr(ws), _numel(ws),
                                          _stream_ptr(terse)))
    return out, status


def decode_binned_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, block: int = BLOCK) -> int:
    return lib().trpx_decode_binned_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block)


def _bin_sides(bin):
    """bin: an int (square bins) or (bin_y, bin_x)"""
    by, bx = (bin, bin) if isinstance(bin, int) else bin
    return int(by), int(bx)


def decode_binned(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, width: int, bin,
                  out_dtype=torch.int32, index: torch.Tensor | None = None, out: torch.Tensor | None = None,
                  workspace: Workspace | None = None, status: torch.Tensor | None = None, block: int = BLOCK):
    """Every frame of a stack resident on the GPU summed over bins of ``bin_y x bin_x`` neighbouring pixels (trpx_decode_binned),
    without decoding its frames to memory: previews, binned diffraction patterns, down-sampled movies.

    ``dtype`` is the stream's pixel type; ``width`` the row length of a frame (``height = n_values // width``); ``bin`` an int
    or ``(bin_y, bin_x)``, each side 1 .. 64 and no larger than the frame's; ``out_dtype`` one of int32, uint32, int64, uint64,
    float32, float64, converted as ``decode_sum`` does.  Returns (binned [n_frames, ceil(height / bin_y), ceil(width / bin_x)],
    status): edge bins sum the pixels that exist, every element is written; asynchronous on the current stream, like ``decode``.
    status[0] is 5 for a corrupt stream or index -- the whole stack is validated.  ``frame_offsets = None``: the frames are
    located first; ``index = None``: the decode index is built on the way (both in ``workspace``)."""
    odt = torch_dtype(out_dtype)
    if odt not in _SUM_OUT:
        raise TypeError(f"decode_binned: out_dtype {odt} (int32, uint32, int64, uint64, float32, float64)")
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    bin_y, bin_x = _bin_sides(bin)
    if width <= 0 or n_values % width:
        raise ValueError(f"decode_binned: width {width} does not divide n_values {n_values}")
    height = n_values // width
    if not (1 <= bin_y <= min(height, 64) and 1 <= bin_x <= min(width, 64)):
        raise ValueError(f"decode_binned: bin {bin_y} x {bin_x} in frames of {height} x {width} (1 .. 64, within the frame)")
    out_h, out_w = -(-height // bin_y), -(-width // bin_x)
    out = _out("decode_binned", out, (n_frames, out_h, out_w), odt, dev)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, False, "binned", code, terse.numel(), n_values, n_frames, block)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_binned(code, _SUM_OUT[odt], terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                       n_values, n_frames, block, width, bin_y, bin_x, out.data_ptr(), status.data_ptr(), _ptr(ws), _numel(ws),
                                       _stream_ptr(terse)))
    return out.view(n_frames, out_h, out_w), status


REDUCE_OPS = {"max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN, "sumsq": _lib.REDUCE_SUMSQ, "count": _lib.REDUCE_COUNT_GE}


def _reduce_op(op) -> int:
    """op: one of "max", "min", "sumsq", "count", or the trpx_reduce_op value"""
    if isinstance(op, str):
        if op not in REDUCE_OPS:
            raise ValueError(f"decode_reduce: op {op!r} (one of {', '.join(REDUCE_OPS)})")
        return REDUCE_OPS[op]
    if int(op) not in REDUCE_OPS.values():
        raise ValueError(f"decode_reduce: op {op!r}")
    return int(op)


def reduce_out_dtype(dtype, op) -> torch.dtype:
    """The element the op writes: the pixel type for max / min, uint64 for sumsq, uint32 for count."""
    code = _reduce_op(op)
    return torch.uint64 if code == _lib.REDUCE_SUMSQ else torch.uint32 if code == _lib.REDUCE_COUNT_GE else torch_dtype(dtype)


def decode_reduce_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, group: int, op, block: int = BLOCK) -> int:
    return lib().trpx_decode_reduce_workspace_bytes(dtype_code(torch_dtype(dtype)), _reduce_op(op), terse_bytes, n_values, n_frames, block, group)


def decode_reduce(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype, group: int, op,
                  threshold: int = 0, out: torch.Tensor | None = None, index: torch.Tensor | None = None,
                  workspace: Workspace | None = None, status: torch.Tensor | None = None, block: int = BLOCK):
    """Per pixel, one statistic over ``group`` consecutive frames of a stack resident on the GPU (trpx_decode_reduce), without
    decoding it to memory.  ``op``: "max" / "min" (elements of the pixel type), "sumsq" (uint64: the sum of squares modulo 2^64)
    or "count" (uint32: the frames with pixel >= ``threshold``).

    ``dtype`` is the stream's pixel type.  Returns (out [ceil(n_frames / group), n_values], status); every element is written;
    asynchronous on the current stream, like ``decode_sum``.  ``frame_offsets = None``: the frames are located first;
    ``index = None``: the decode index is built on the way."""
    code, opc = dtype_code(torch_dtype(dtype)), _reduce_op(op)
    odt = reduce_out_dtype(dtype, opc)
    dev = terse.device
    n_out = -(-n_frames // group) if group > 0 else 0
    out = _out("decode_reduce", out, (n_out, n_values), odt, dev)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "reduce", code, opc, terse.numel(), n_values, n_frames, block, group)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_reduce(code, opc, terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index), n_values, n_frames,
                                       block, group, int(threshold), out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream_ptr(terse)))
    return out, status


def decode_sum_labelled_workspace_bytes(terse_bytes: int, n_values: int, n_frames: int, dtype, n_out: int, block: int = BLOCK) -> int:
    return lib().trpx_decode_sum_labelled_workspace_bytes(dtype_code(torch_dtype(dtype)), terse_bytes, n_values, n_frames, block, n_out)


def decode_sum_labelled(terse: torch.Tensor, frame_offsets: torch.Tensor | None, n_values: int, n_frames: int, dtype,
                        labels: torch.Tensor, n_out: int, out_dtype=torch.int32, out: torch.Tensor | None = None,
                        counts: torch.Tensor | None = None, index: torch.Tensor | None = None,
                        workspace: Workspace | None = None, status: torch.Tensor | None = None, block: int = BLOCK):
    """Sums of the frames that carry the same label, of a stack resident on the GPU (trpx_decode_sum_labelled), without decoding
    it to memory.  ``labels``: one uint32 (or int32, read as uint32: -1 is the mask) per frame, on the device; frame f is added
    into output ``labels[f]``, a label >= ``n_out`` takes the frame out of every sum and it is not read.

    ``dtype`` is the stream's pixel type; ``out_dtype`` one of int32, uint32, int64, uint64, float32, float64.  Returns
    (sums [n_out, n_values], status); every element is written, an output without frames is 0.  ``counts``: a uint32 (or
    int32) tensor of n_out elements that receives the frames per output.  Asynchronous on the current stream, like
    ``decode_sum``.  ``frame_offsets = None``: the frames are located first; ``index = None``: the decode index is built on the way."""
    odt = torch_dtype(out_dtype)
    if odt not in _SUM_OUT:
        raise TypeError(f"decode_sum_labelled: out_dtype {odt} (int32, uint32, int64, uint64, float32, float64)")
    code = dtype_code(torch_dtype(dtype))
    dev = terse.device
    words = (torch.uint32, torch.int32)
    if labels.dtype not in words or labels.numel() != n_frames or not labels.is_contiguous() or labels.device != dev:
        raise ValueError(f"decode_sum_labelled: labels must be a contiguous uint32 / int32 tensor of {n_frames} elements on {dev}")
    if counts is not None and (counts.dtype not in words or counts.numel() != n_out or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"decode_sum_labelled: counts must be a contiguous uint32 / int32 tensor of {n_out} elements on {dev}")
    out = _out("decode_sum_labelled", out, (n_out, n_values), odt, dev)
    status = _status(status, dev)
    ws = _consumer_ws(workspace, dev, frame_offsets, index, True, "sum_labelled", code, terse.numel(), n_values, n_frames, block, n_out)
    with torch.cuda.device(dev):
        check(lib().trpx_decode_sum_labelled(code, _SUM_OUT[odt], terse.data_ptr(), terse.numel(), _ptr(frame_offsets), _ptr(index),
                                             n_values, n_frames, block, labels.data_ptr(), n_out, out.data_ptr(), _ptr(counts),
                                             status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(terse)))
    return out, status


def select_frames_workspace_bytes(n_frames: int, n_select: int) -> int:
    return lib().trpx_select_frames_workspace_bytes(n_frames, n_select)


def select_frames(terse: torch.Tensor, frame_offsets: torch.Tensor, frames: torch.Tensor, n_values: int, n_frames: int, dtype,
                  index: torch.Tensor | None = None, out: torch.Tensor | None = None, workspace: Workspace | None = None,
                  status: torch.Tensor | None = None, out_offsets: torch.Tensor | None = None, block: int = BLOCK) -> Encoded:
    """The frames ``frames`` of a stack resident on the GPU as a new stack (trpx_select_frames), without decoding them: the
    result is byte for byte what ``encode`` writes for ``pixels[frames]``.  Only bytes move, so every block size and every
    integer dtype is taken; ``dtype``, ``n_values`` and ``block`` matter only for the index.

    ``frames``: a contiguous uint32 / int32 device tensor, any order, repeats allowed, possibly longer than the stack;
    ``frame_offsets`` is mandatory (``locate_frames`` for an index-free stack).  With ``index`` (the source's decode index; block
    12, pixels of up to 32 bits) the result carries ``.index``, its own decode index.  Returns an ``Encoded`` of ``len(frames)``
    frames; ``Encoded.check()`` (synchronises) raises on status[0]: 1 for an entry that is no frame of the stack, 5 for a selected
    frame whose offsets decrease or leave the stream, 3 when ``out`` is too small (the offsets are still complete).  status[1]
    is 0: the call does not know prolix_bits.

    With ``out`` given: ONE call, asynchronous on the current stream (capturable into a graph; a replay takes a new list from
    the same ``frames`` buffer).  With ``out=None`` the call SYNCHRONISES: a sizes-only call, one read of the total, a tensor of
    its own, a second call.  ``out`` must not overlap ``terse``."""
    tdt = torch_dtype(dtype)
    code = dtype_code(tdt)
    dev = terse.device
    if not terse.is_cuda:
        raise ValueError("select_frames: the stack must live on the GPU (use trpx_amd.Terse.select for host data)")
    if frames.dtype not in (torch.uint32, torch.int32) or frames.dim() != 1 or not frames.is_contiguous() or frames.device != dev:
        raise TypeError(f"select_frames: frames must be a contiguous 1-d uint32 / int32 tensor on {dev}")
    n_select = frames.numel()
    if out_offsets is None:
        out_offsets = torch.empty(n_select + 1, dtype=torch.int64, device=dev)
    status = _status(status, dev)
    ws = _scratch(workspace, dev, select_frames_workspace_bytes(n_frames, n_select))
    out_index = None
    if index is not None:
        out_index = torch.empty(index_bytes(tdt, n_values, n_select, block), dtype=torch.uint8, device=dev)

    def call(o):
        with torch.cuda.device(dev):
            check(lib().trpx_select_frames(code, terse.data_ptr(), terse.numel(), frame_offsets.data_ptr(), _ptr(index), n_values,
                                           n_frames, block, frames.data_ptr(), n_select, _ptr(o), o.numel() if o is not None else 0,
                                           out_offsets.data_ptr(), _ptr(out_index), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _stream_ptr(terse)))

    if out is None:
        call(None)
        total = int(out_offsets[-1].item())                  # (synchronises)
        if int(status[0].item()) in (_lib.OK, _lib.ERR_CAPACITY):
            out = torch.empty(max((total + 15) // 16 * 16, 16), dtype=torch.uint8, device=dev)
    if out is not None:
        call(out)
    else:
        out = torch.empty(0, dtype=torch.uint8, device=dev)
    return Encoded(out, out_offsets, status, n_values, n_select, tdt, out_index)
