"""Host-side mirror of the reference class ``jpa::Terse`` (include/Terse.hpp:228-475).

Same surface and argument meaning -- construct from data, ``push_back`` frames, ``prolix`` a
frame into caller memory, ``write`` / read the ``.trpx`` stream -- but every encode / decode runs
on the MI355X through the C ABI (``trpx_encode_host`` / ``trpx_decode_host``).  The compressed
bytes live on the host, as in the reference (``d_terse_data``, Terse.hpp:482).  The C++ mirror
of the same class is ``include/trpx/Terse.hpp``.

Differences, all deliberate:
  * frames are located by the running sum of their sizes (the *intended* semantics of
    Terse.hpp:562-585; the reference's cached offsets are wrong for frame >= 2, defect D1);
  * argument errors raise ``ValueError`` where the reference ``assert``s (compiled out in its
    Release build);
  * ``push_back_stack`` / ``prolix_stack`` move many frames in one GPU call (no O(F^2), D6).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

_NP2DT = {np.dtype(np.uint8): _lib.U8, np.dtype(np.int8): _lib.I8, np.dtype(np.uint16): _lib.U16,
          np.dtype(np.int16): _lib.I16, np.dtype(np.uint32): _lib.U32, np.dtype(np.int32): _lib.I32,
          np.dtype(np.uint64): _lib.U64, np.dtype(np.int64): _lib.I64}


_NP2DT_OUT = dict(_NP2DT)
_NP2DT_OUT.update({np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64})


def _code(dt, decode: bool = False) -> int:
    try:
        return (_NP2DT_OUT if decode else _NP2DT)[np.dtype(dt)]
    except KeyError:
        raise TypeError(f"Terse: unsupported pixel type {dt} (encode: u8/i8/u16/i16/u32/i32/u64/i64; decode also "
                        f"float32/float64)") from None


class Terse:
    def __init__(self, data=None, block: int = 12, device: int = -1):
        """``Terse()`` (Terse.hpp:237) or ``Terse(container)`` (Terse.hpp:249-253, :263-270)."""
        self._block = int(block)
        self._device = device
        self._signed = False
        self._size = 0
        self._prolix_bits = 0
        self._dim: list[int] = []
        self._data = bytearray()
        self._stack, self._stack_len = None, -1      # device-resident copy of the stack (prolix), see _drop_stack
        self._group_states = None                    # chain state at every 256th block of every frame (row f1), or None
        self._frame_sizes: list[int] = []
        if data is not None:
            self.push_back(data)

    # ---- encode -----------------------------------------------------------------------------
    def push_back(self, data) -> None:
        """Append one frame (Terse.hpp:290-302, :312-322)."""
        a = np.ascontiguousarray(data)
        if a.ndim > 1:
            if not self._frame_sizes and not self._dim:
                self._dim = list(a.shape)                   # captures dim() (Terse.hpp:251-252, :314-317)
            elif self._dim and list(a.shape) != self._dim:
                raise ValueError("each frame of a multi-Terse object must have the same dimensions")  # :319
        self.push_back_stack(a.reshape(1, -1))

    def push_back_stack(self, frames) -> None:
        """Append a [n_frames, ...] stack in ONE GPU call (what a detector pipeline would do)."""
        a = np.ascontiguousarray(frames)
        a = a.reshape(a.shape[0], -1)
        if a.dtype in (np.dtype(np.int64), np.dtype(np.uint64)):
            # 64-bit integers (what src/terse.cpp:120-123 makes of float images): values that fit 32 bits give the same
            # stream whatever the container type, so they are narrowed here and take the tuned kernels; a stack with wider
            # values goes through as 64-bit pixels (generic kernels, fields of up to 64 bits)
            narrow = np.int32 if a.dtype.kind == "i" else np.uint32
            if not (a.size and (a.min() < np.iinfo(narrow).min or a.max() > np.iinfo(narrow).max)):
                a = a.astype(narrow)
        code = _code(a.dtype)
        n_frames, n = a.shape
        if n_frames == 0:
            return
        if self._frame_sizes:
            if n != self._size:
                raise ValueError("each frame of a multi-Terse object must have the same size")   # Terse.hpp:297
            if (a.dtype.kind == "i") != self._signed:
                raise ValueError("signedness differs from the first frame")                      # Terse.hpp:298
        cap = n_frames * lib().trpx_worst_case_bytes(code, n, self._block)
        out = np.empty(cap, np.uint8)
        total = C.c_size_t(0)
        offs = np.empty(n_frames + 1, np.uint64)
        pb = C.c_uint(0)
        check(lib().trpx_encode_host(code, a.ctypes.data, n, n_frames, self._block, out.ctypes.data, cap,
                                     C.byref(total), offs.ctypes.data, C.byref(pb), self._device))
        if not self._frame_sizes:
            self._size = n
            self._signed = a.dtype.kind == "i"
        self._data += out[: total.value].tobytes()
        self._group_states = None
        self._frame_sizes += [int(x) for x in np.diff(offs)]
        self._prolix_bits = max(self._prolix_bits, int(pb.value))   # Terse.hpp:516

    def push_back_sparse(self, row_offsets, positions, values, size: int | None = None) -> None:
        """Append frames given as their events in CSR form, in ONE GPU call (trpx_encode_sparse_host), without building the
        dense frames: frame k is ``size()`` zeros with ``px[positions[i]] = values[i]`` for ``row_offsets[k] <= i <
        row_offsets[k + 1]`` -- what ``prolix_sparse`` returns.  Positions ascend strictly inside a frame (``ValueError``
        otherwise).  The pixel type is that of ``values``; on the first push the frame size is ``size``, or the product of
        ``dim()``.  Afterwards the object is what ``push_back_stack`` of the dense frames makes of it."""
        rows = np.ascontiguousarray(np.asarray(row_offsets), dtype=np.uint64)
        pos = np.ascontiguousarray(np.asarray(positions), dtype=np.uint32).reshape(-1)
        val = np.ascontiguousarray(values).reshape(-1)
        code = _code(val.dtype)
        n_frames = rows.size - 1
        if rows.ndim != 1 or n_frames < 0 or pos.size != val.size:
            raise ValueError("push_back_sparse: row_offsets [n_frames + 1], positions and values of one length")
        if n_frames == 0:
            return
        if self._frame_sizes:
            if size is not None and int(size) != self._size:
                raise ValueError("each frame of a multi-Terse object must have the same size")   # Terse.hpp:297
            if (val.dtype.kind == "i") != self._signed:
                raise ValueError("signedness differs from the first frame")                      # Terse.hpp:298
            n = self._size
        else:
            n = int(size) if size is not None else int(np.prod(self._dim)) if self._dim else 0
            if n <= 0:
                raise ValueError("push_back_sparse: the first push needs the frame size (size=, or dim())")
        cap = lib().trpx_encode_sparse_bound_bytes(code, n, n_frames, pos.size, self._block)
        if cap == 0:
            raise ValueError("push_back_sparse: block 12, pixels of <= 32 bits and frames of < 2^32 values only")
        out = np.empty(cap, np.uint8)
        total = C.c_size_t(0)
        offs = np.empty(n_frames + 1, np.uint64)
        pb = C.c_uint(0)
        rc = lib().trpx_encode_sparse_host(code, rows.ctypes.data, pos.ctypes.data if pos.size else None,
                                           val.ctypes.data if pos.size else None, pos.size, n, n_frames, self._block,
                                           out.ctypes.data, cap, C.byref(total), offs.ctypes.data, C.byref(pb), self._device)
        if rc == _lib.ERR_INVALID_ARG:
            raise ValueError(lib().trpx_last_error_string().decode(errors="replace"))
        check(rc)
        if not self._frame_sizes:
            self._size = n
            self._signed = val.dtype.kind == "i"
        self._data += out[: total.value].tobytes()
        self._group_states = None
        self._frame_sizes += [int(x) for x in np.diff(offs)]
        self._prolix_bits = max(self._prolix_bits, int(pb.value))   # Terse.hpp:516

    # ---- decode -----------------------------------------------------------------------------
    def prolix(self, out: np.ndarray, frame: int = 0) -> np.ndarray:
        """Unpack frame `frame` into `out` (Terse.hpp:333-341, :352-389).  `out` may have any supported type:
        narrower integers clamp (Bit_pointer.hpp:747-763), float / double are exact (Terse.hpp:379-383)."""
        if not 0 <= frame < self.number_of_frames():
            raise ValueError("frame index out of range")                                          # Terse.hpp:354
        if out.size != self._size:
            raise ValueError("output container has the wrong size")                               # Terse.hpp:335
        if self._signed and out.dtype.kind == "u":
            raise ValueError("signed data cannot be decompressed into unsigned data")            # Terse.hpp:356-357
        if not out.flags.c_contiguous:
            raise ValueError("output must be contiguous")
        # src/prolix.cpp:69-92 calls this once per frame: the stack is uploaded once and kept on the device (trpx_stack_*),
        # a window of frames is expanded per device call and a call normally only copies its frame back
        if self._stack is None or self._stack_len != len(self._data):
            self._drop_stack()
            buf, offs = self._stream_and_offsets()
            h = C.c_void_p()
            gs = self._states()
            check(lib().trpx_stack_open(C.byref(h), int(self._signed), buf.ctypes.data, buf.size, offs.ctypes.data,
                                        gs.ctypes.data if gs is not None else None, self._size,
                                        len(self._frame_sizes), self._block, 0, self._device))
            self._stack, self._stack_len = h, len(self._data)
        check(lib().trpx_stack_read(self._stack, frame, _code(out.dtype, True), out.ctypes.data))
        return out

    def _states(self):
        """The group states if they belong to the object's current frames, else None."""
        groups = lib().trpx_group_count(self._size, self._block) if self._size else 0
        gs = self._group_states
        return gs if gs is not None and groups and gs.size == groups * len(self._frame_sizes) else None

    def has_group_index(self) -> bool:
        return self._states() is not None

    def _drop_stack(self) -> None:
        if getattr(self, "_stack", None) is not None:
            lib().trpx_stack_close(self._stack)
        self._stack, self._stack_len = None, -1

    def __del__(self):
        try:
            self._drop_stack()
        except Exception:
            pass

    # The device-side copy of the stack (a raw trpx_stack*) belongs to ONE object: copies and pickles start without it.
    def __getstate__(self):
        st = dict(self.__dict__)
        st["_stack"], st["_stack_len"] = None, -1
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._stack, self._stack_len = None, -1

    def __copy__(self):
        t = Terse.__new__(Terse)
        t.__setstate__(self.__getstate__())
        return t

    def __deepcopy__(self, memo):
        import copy
        t = Terse.__new__(Terse)
        t.__setstate__({k: copy.deepcopy(v, memo) for k, v in self.__getstate__().items()})
        return t

    def prolix_stack(self, dtype) -> np.ndarray:
        """Decode every frame in ONE GPU call; returns [n_frames, size]."""
        f = self.number_of_frames()
        out = np.empty((f, self._size), np.dtype(dtype))
        buf, offs = self._stream_and_offsets()
        gs = self._states()
        check(lib().trpx_decode_host_grouped(int(self._signed), _code(dtype, True), buf.ctypes.data, buf.size, offs.ctypes.data,
                                             gs.ctypes.data if gs is not None else None, self._size, f, self._block,
                                             out.ctypes.data, self._device))
        return out

    def prolix_sum(self, group: int | None = None, dtype=np.int64) -> np.ndarray:
        """Sums of ``group`` consecutive frames (``None``: all frames) in ONE GPU call (trpx_decode_sum_host), without
        decoding the stack to memory; returns [ceil(number_of_frames / group), size] of ``dtype`` (int32 / uint32 clamp,
        int64 / uint64 exact, float32 / float64 rounded once)."""
        f = self.number_of_frames()
        if group is None:
            group = f
        if group < 1:
            raise ValueError("group must be >= 1")
        if self._signed and np.dtype(dtype).kind == "u":
            raise ValueError("signed data cannot be decompressed into unsigned data")            # Terse.hpp:356-357
        stream, _ = self._stream_type("prolix_sum")
        out = np.empty((-(-f // group) if f else 0, self._size), np.dtype(dtype))
        if f == 0:
            return out
        buf, offs = self._stream_and_offsets()
        check(lib().trpx_decode_sum_host(stream, _code(dtype, True), buf.ctypes.data, buf.size, offs.ctypes.data, self._size,
                                         f, self._block, group, out.ctypes.data, self._device))
        return out

    def prolix_sum_labelled(self, labels, n_out: int | None = None, dtype=np.int64, return_counts: bool = False):
        """Sums of the frames that carry the same label in ONE GPU call (trpx_decode_sum_labelled_host), without decoding the
        stack to memory.  ``labels``: one unsigned 32-bit label per frame; frame f is added into output ``labels[f]``, a label
        >= ``n_out`` (by convention 2^32 - 1) takes the frame out of every sum.  ``n_out`` defaults to the largest label below
        2^32 - 1, plus one.  Returns [n_out, size] of ``dtype`` (int32 / uint32 clamp, int64 / uint64 exact, float32 / float64
        rounded once), an output without frames is 0; with ``return_counts`` also the frames per output (uint32 [n_out])."""
        f = self.number_of_frames()
        lab = np.asarray(labels)
        if lab.shape != (f,) or lab.dtype.kind not in "iu" or (lab.size and (lab.min() < 0 or lab.max() > 0xFFFFFFFF)):
            raise ValueError(f"prolix_sum_labelled: labels must be {f} integers in [0, 2^32)")
        lab = np.ascontiguousarray(lab, np.uint32)
        if n_out is None:
            kept = lab[lab != 0xFFFFFFFF]
            n_out = int(kept.max()) + 1 if kept.size else 1
        if n_out < 1:
            raise ValueError("n_out must be >= 1")
        if self._signed and np.dtype(dtype).kind == "u":
            raise ValueError("signed data cannot be decompressed into unsigned data")            # Terse.hpp:356-357
        stream, _ = self._stream_type("prolix_sum_labelled")
        out = np.zeros((n_out, self._size), np.dtype(dtype))
        counts = np.zeros(n_out, np.uint32)
        if f:
            buf, offs = self._stream_and_offsets()
            check(lib().trpx_decode_sum_labelled_host(stream, _code(dtype, True), buf.ctypes.data, buf.size, offs.ctypes.data, self._size,
                                                      f, self._block, lab.ctypes.data, n_out, out.ctypes.data, counts.ctypes.data,
                                                      self._device))
        return (out, counts) if return_counts else out

    def prolix_reduce(self, op: str, group: int | None = None, threshold: int = 0) -> np.ndarray:
        """Per pixel, one statistic over ``group`` consecutive frames (``None``: all frames) in ONE GPU call
        (trpx_decode_reduce_host), without decoding the stack to memory.  ``op``: ``"max"`` / ``"min"`` (elements of the
        narrowest integer type that holds the object's values), ``"sumsq"`` (uint64: the sum of squares modulo 2^64; with
        ``prolix_sum`` the per-pixel variance) or ``"count"`` (uint32: the frames with pixel >= ``threshold``).  Returns
        [ceil(number_of_frames / group), size]."""
        ops = {"max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN, "sumsq": _lib.REDUCE_SUMSQ, "count": _lib.REDUCE_COUNT_GE}
        if op not in ops:
            raise ValueError(f"prolix_reduce: op {op!r} (one of {', '.join(ops)})")
        f = self.number_of_frames()
        if group is None:
            group = f
        if f and group < 1:
            raise ValueError("group must be >= 1")
        code, dt = self._stream_type("prolix_reduce")
        out = np.empty((-(-f // group) if f else 0, self._size), {"sumsq": np.dtype(np.uint64), "count": np.dtype(np.uint32)}.get(op, dt))
        if f == 0:
            return out
        buf, offs = self._stream_and_offsets()
        check(lib().trpx_decode_reduce_host(code, ops[op], buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f, self._block,
                                            group, int(threshold), out.ctypes.data, self._device))
        return out

    def _stream_and_offsets(self):
        """The stream and its frame offsets as the host entry points take them: (uint8 array, uint64 [frames + 1])."""
        return np.frombuffer(self._data, np.uint8), np.concatenate([[0], np.cumsum(self._frame_sizes)]).astype(np.uint64)

    def _stream_type(self, what: str):
        """The narrowest stream type that holds the object's values: (dtype code, numpy dtype)."""
        if self._prolix_bits > 32:
            raise ValueError(f"{what}: values of more than 32 bits are not supported")
        bits = 8 if self._prolix_bits <= 8 else 16 if self._prolix_bits <= 16 else 32
        code = {8: _lib.U8, 16: _lib.U16, 32: _lib.U32}[bits] + int(self._signed)
        return code, np.dtype(f"{'i' if self._signed else 'u'}{bits // 8}")

    def prolix_boxes(self, boxes, shape) -> np.ndarray:
        """Boxes of pixels in ONE GPU call (trpx_decode_roi_host), without decoding whole frames to memory.  ``boxes``: rows
        ``(frame, y0, x0)``, in any order, overlapping or repeated; ``shape = (h, w)`` for all of them.  ``dim()`` =
        {width, height} must be set.  Returns [len(boxes), h, w] of the narrowest integer type that holds the object's values."""
        if len(self._dim) != 2 or self._dim[0] * self._dim[1] != self._size:
            raise ValueError("prolix_boxes: dim() must be set to {width, height} of the frames")
        width, height = self._dim
        h, w = (int(x) for x in shape)
        b = np.asarray(boxes, dtype=np.int64).reshape(-1, 3)
        if not (1 <= h <= height and 1 <= w <= width):
            raise ValueError("prolix_boxes: the box shape does not fit the frame")
        if b.size and (b.min() < 0 or (b[:, 0] >= self.number_of_frames()).any() or (b[:, 1] + h > height).any() or (b[:, 2] + w > width).any()):
            raise ValueError("prolix_boxes: a box leaves the stack")
        code, dt = self._stream_type("prolix_boxes")
        out = np.empty((b.shape[0], h, w), dt)
        if b.shape[0] == 0:
            return out
        b32 = np.ascontiguousarray(b, dtype=np.uint32)
        buf, offs = self._stream_and_offsets()
        check(lib().trpx_decode_roi_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, self._size, self.number_of_frames(),
                                         self._block, width, b32.ctypes.data, b32.shape[0], h, w, out.ctypes.data, self._device))
        return out

    def prolix_roi(self, y0: int, x0: int, h: int, w: int, frames=None) -> np.ndarray:
        """The same rectangle of every frame in ``frames`` (default: all): [len(frames), h, w] (see ``prolix_boxes``)."""
        frames = range(self.number_of_frames()) if frames is None else frames
        return self.prolix_boxes([(int(f), y0, x0) for f in frames], (h, w))

    def prolix_binned(self, bin, out_dtype=np.int32) -> np.ndarray:
        """Every frame summed over bins of ``bin_y x bin_x`` neighbouring pixels in ONE GPU call (trpx_decode_binned_host),
        without decoding the frames to memory.  ``bin``: an int or ``(bin_y, bin_x)``, each side 1 .. 64 and no larger than the
        frame's; ``dim()`` = {width, height} must be set.  Returns ``[number_of_frames, ceil(height / bin_y), ceil(width /
        bin_x)]`` of ``out_dtype`` (int32 / uint32 clamp, int64 / uint64 exact, float32 / float64 rounded once); edge bins sum
        the pixels that exist."""
        if len(self._dim) != 2 or self._dim[0] * self._dim[1] != self._size:
            raise ValueError("prolix_binned: dim() must be set to {width, height} of the frames")
        width, height = self._dim
        bin_y, bin_x = (int(bin), int(bin)) if np.isscalar(bin) else (int(x) for x in bin)
        if not (1 <= bin_y <= min(height, 64) and 1 <= bin_x <= min(width, 64)):
            raise ValueError("prolix_binned: a bin side is 1 .. 64 and no larger than the frame's")
        if self._signed and np.dtype(out_dtype).kind == "u":
            raise ValueError("signed data cannot be decompressed into unsigned data")            # Terse.hpp:356-357
        code, _ = self._stream_type("prolix_binned")
        f = self.number_of_frames()
        out = np.empty((f, -(-height // bin_y), -(-width // bin_x)), np.dtype(out_dtype))
        if f:
            buf, offs = self._stream_and_offsets()
            check(lib().trpx_decode_binned_host(code, _code(out_dtype, True), buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f,
                                                self._block, width, bin_y, bin_x, out.ctypes.data, self._device))
        return out

    def prolix_sparse(self, threshold: int, frames=None):
        """The pixels with value >= ``threshold`` (trpx_decode_sparse_host: two GPU calls, sizes then events), without decoding
        the frames to memory.  Returns numpy ``(row_offsets int64 [n + 1], positions uint32, values)``: event i of the k-th frame
        asked for, row_offsets[k] <= i < row_offsets[k + 1], is pixel positions[i] of that frame with value values[i], in ascending
        pixel order; values have the narrowest integer type that holds the object's values.  ``frames``: a list of frame numbers
        (default: all), results in the order asked."""
        code, dt = self._stream_type("prolix_sparse")
        f = self.number_of_frames()
        frames = list(range(f)) if frames is None else [int(x) for x in frames]
        if any(x < 0 or x >= f for x in frames):
            raise ValueError("prolix_sparse: frame index out of range")
        rows = np.zeros(f + 1, np.uint64)
        pos, val = np.empty(0, np.uint32), np.empty(0, dt)
        if f:
            buf, offs = self._stream_and_offsets()
            found = C.c_size_t(0)

            def call(p, v, cap):
                return lib().trpx_decode_sparse_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f, self._block,
                                                     int(threshold), rows.ctypes.data, p, v, cap, C.byref(found), self._device)
            rc = call(None, None, 0)
            if rc != _lib.ERR_CAPACITY:                      # (CAPACITY: there are events, found.value of them)
                check(rc)
            if found.value:
                pos, val = np.empty(found.value, np.uint32), np.empty(found.value, dt)
                check(call(pos.ctypes.data, val.ctypes.data, found.value))
        rows = rows.astype(np.int64)
        if frames == list(range(f)):
            return rows, pos, val
        pieces = [slice(int(rows[x]), int(rows[x + 1])) for x in frames]     # (the whole stack is decoded: filtered on the host)
        out_rows = np.concatenate([[0], np.cumsum([p.stop - p.start for p in pieces])]).astype(np.int64)
        if not pieces:
            return out_rows, pos[:0], val[:0]
        return out_rows, np.concatenate([pos[p] for p in pieces]), np.concatenate([val[p] for p in pieces])

    def prolix_dot(self, weights) -> np.ndarray:
        """Per frame the sums of its pixels weighted by K integer maps in ONE GPU call (trpx_decode_dot_host), without decoding
        the frames to memory.  ``weights``: int32 ``[K, size]`` (or ``[K, H, W]`` with ``H * W == size``, or one map), 1 <= K <=
        16.  Returns int64 ``[number_of_frames, K]``: ``[f, k] = sum_p px[f][p] * weights[k][p]``, exact, modulo 2^64 -- a mask
        gives a virtual detector image, the maps x, y and 1 the centre of mass."""
        w = np.asarray(weights)
        if w.dtype.kind not in "iu" or (w.size and (w.min() < -2**31 or w.max() > 2**31 - 1)):
            raise TypeError("prolix_dot: weights must be integers that fit int32")
        if w.ndim == 1:
            w = w[None]
        if w.ndim < 2 or w.size != w.shape[0] * self._size or not 1 <= w.shape[0] <= 16:
            raise ValueError("prolix_dot: weights must be [K, size] or [K, H, W] with 1 <= K <= 16")
        w = np.ascontiguousarray(w.reshape(w.shape[0], self._size), dtype=np.int32)
        code, _ = self._stream_type("prolix_dot")
        f = self.number_of_frames()
        out = np.zeros((f, w.shape[0]), np.int64)
        if f:
            buf, offs = self._stream_and_offsets()
            check(lib().trpx_decode_dot_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f, self._block,
                                             w.ctypes.data, w.shape[0], out.ctypes.data, self._device))
        return out

    def prolix_bins(self, labels, n_bins: int) -> np.ndarray:
        """Per frame the sums of its pixels over the bins of a label map in ONE GPU call (trpx_decode_bins_host), without
        decoding the frames to memory.  ``labels``: integers ``[size]`` (or ``[H, W]`` with ``H * W == size``) that fit uint16;
        a label >= n_bins belongs to no bin (mask with 0xFFFF); 1 <= n_bins <= 4096.  Returns int64 ``[number_of_frames,
        n_bins]``: ``[f, b] = sum of px[f][p] over labels[p] == b``, exact -- the radial profile of every frame."""
        lab = np.asarray(labels)
        if lab.dtype.kind not in "iu" or (lab.size and (lab.min() < 0 or lab.max() > 0xFFFF)):
            raise TypeError("prolix_bins: labels must be integers that fit uint16")
        if lab.size != self._size:
            raise ValueError("prolix_bins: labels must be [size] or [H, W]")
        if not 1 <= int(n_bins) <= 4096:
            raise ValueError("prolix_bins: 1 to 4096 bins")
        lab = np.ascontiguousarray(lab.reshape(self._size), dtype=np.uint16)
        code, _ = self._stream_type("prolix_bins")
        f = self.number_of_frames()
        out = np.zeros((f, int(n_bins)), np.int64)
        if f:
            buf, offs = self._stream_and_offsets()
            check(lib().trpx_decode_bins_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f, self._block,
                                              lab.ctypes.data, int(n_bins), out.ctypes.data, self._device))
        return out

    def prolix_hist(self, group: int = 1, lo: int = 0, shift: int = 0, n_bins: int = 256) -> np.ndarray:
        """Per group of ``group`` consecutive frames the histogram of its pixel values in ONE GPU call (trpx_decode_hist_host),
        without decoding the frames to memory: ``bin(v) = clamp((v - lo) >> shift, 0, n_bins - 1)``, the first and the last bin
        taking everything below and above.  1 <= n_bins <= 4096, 0 <= shift <= 32, |lo| <= 2^32, group >= 1 (the last group holds
        what is left).  Returns int64 ``[ceil(number_of_frames / group), n_bins]``: exact counts, each row summing to size() x the
        group's frames -- ``np.bincount(np.clip((px.astype(np.int64) - lo) >> shift, 0, n_bins - 1).ravel(), minlength=n_bins)``."""
        group, lo, shift, n_bins = int(group), int(lo), int(shift), int(n_bins)
        if not 1 <= n_bins <= 4096:
            raise ValueError("prolix_hist: 1 to 4096 bins")
        if not 0 <= shift <= 32 or abs(lo) > 2**32:
            raise ValueError("prolix_hist: 0 <= shift <= 32 and |lo| <= 2^32")
        if group < 1:
            raise ValueError("prolix_hist: group >= 1")
        code, _ = self._stream_type("prolix_hist")
        f = self.number_of_frames()
        out = np.zeros((-(-f // min(group, f)) if f else 0, n_bins), np.uint64)
        if f:
            buf, offs = self._stream_and_offsets()
            check(lib().trpx_decode_hist_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f, self._block, group, lo,
                                              shift, n_bins, out.ctypes.data, self._device))
        return out.astype(np.int64)

    def prolix_corrected(self, dark=None, gain=None, first: int = 0, n: int | None = None) -> np.ndarray:
        """Frames ``[first, first + n)`` (``n = None``: to the end) as float32 with the dark reference subtracted and the gain
        reference multiplied in, in ONE GPU call (trpx_decode_corrected_host): ``(px.astype(np.float32) - dark) * gain``, three
        float32 operations in this order, each rounded once; subnormal results are unspecified.  ``dark`` / ``gain``: size()
        values (any shape, converted to float32), or None to leave the operation out.  Returns float32 ``[n, size()]``."""
        f = self.number_of_frames()
        first = int(first)
        n = f - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > f:
            raise ValueError("prolix_corrected: frames out of range")
        maps = []
        for name, m in (("dark", dark), ("gain", gain)):
            if m is not None:
                m = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(-1))
                if m.size != self._size:
                    raise ValueError(f"prolix_corrected: {name} must hold size() values")
            maps.append(m)
        code, _ = self._stream_type("prolix_corrected")
        out = np.empty((n, self._size), np.float32)
        if n:
            buf, offs = self._stream_and_offsets()
            a, b = int(offs[first]), int(offs[first + n])
            sub = np.ascontiguousarray(buf[a:b])
            rel = np.ascontiguousarray(offs[first:first + n + 1] - offs[first])
            check(lib().trpx_decode_corrected_host(code, _lib.F32, sub.ctypes.data, sub.size, rel.ctypes.data, self._size, n, self._block,
                                                   maps[0].ctypes.data if maps[0] is not None else None,
                                                   maps[1].ctypes.data if maps[1] is not None else None, out.ctypes.data, self._device))
        return out

    def select(self, frames) -> "Terse":
        """A new object holding the frames ``frames`` of this one, in ONE GPU call (trpx_select_frames_host), without decoding
        them: the frames' bytes are copied, so the result is what ``push_back_stack(pixels[frames])`` would make.  ``frames``: a
        sequence of frame numbers -- any order, repeats allowed, possibly longer than the stack -- or a boolean mask of
        ``number_of_frames()`` entries.  ``dim()``, signedness and block are copied; ``bits_per_val()`` is kept from the source and
        is therefore an UPPER BOUND for the selected frames (the call never looks at a pixel)."""
        f = self.number_of_frames()
        idx = np.asarray(frames)
        if idx.dtype == np.bool_:
            if idx.shape != (f,):
                raise ValueError("select: a mask needs one entry per frame")
            idx = np.flatnonzero(idx)
        idx = idx.reshape(-1)
        if idx.size and (idx.dtype.kind not in "iu" or idx.min() < 0 or idx.max() >= f):
            raise ValueError("select: frame index out of range")
        t = Terse(block=self._block, device=self._device)
        t._signed, t._size, t._prolix_bits, t._dim = self._signed, self._size, self._prolix_bits, list(self._dim)
        if idx.size == 0:
            return t
        idx32 = np.ascontiguousarray(idx, dtype=np.uint32)
        buf, offs = self._stream_and_offsets()
        sizes = np.diff(offs)[idx32]
        out = np.empty(int(sizes.sum()), np.uint8)
        out_offs = np.empty(idx32.size + 1, np.uint64)
        total = C.c_size_t(0)
        check(lib().trpx_select_frames_host(_lib.U8 + int(self._signed), buf.ctypes.data, buf.size, offs.ctypes.data, self._size, f,
                                            self._block, idx32.ctypes.data, idx32.size, out.ctypes.data, out.size,
                                            out_offs.ctypes.data, C.byref(total), self._device))
        t._data = bytearray(out[: total.value].tobytes())
        t._frame_sizes = [int(x) for x in np.diff(out_offs)]
        gs = self._states()
        if gs is not None:
            t._group_states = np.ascontiguousarray(gs.reshape(f, -1)[idx32]).reshape(-1)
        return t

    # ---- accessors (Terse.hpp:396-444) --------------------------------------------------------
    def size(self) -> int:
        return self._size

    def number_of_frames(self) -> int:
        return len(self._frame_sizes)

    def is_signed(self) -> bool:
        return self._signed

    def bits_per_val(self) -> int:
        return self._prolix_bits

    def terse_size(self) -> int:
        return len(self._data)

    def imagej_readable(self) -> bool:
        """True if the reference's ImageJ plugin accepts a file written from this object: it only reads unsigned data
        of at most 16 bits per value (ImageJ/TRPX_Reader.java:94-98) and the whole file must fit a Java byte array."""
        return (not self._signed) and self._prolix_bits <= 16 and len(self._data) < (1 << 31) - 4096

    def frame_sizes(self) -> list[int]:
        return list(self._frame_sizes)

    def data(self) -> bytes:
        return bytes(self._data)

    def dim(self, dim=None):
        if dim is not None:
            if self._dim:
                raise ValueError("you cannot overwrite the dimensionality of a frame")           # Terse.hpp:419
            self._dim = [int(d) for d in dim]
        return list(self._dim)

    # ---- stream-serialise surface (Terse.hpp:454-474, :279, :485-498) -----------------------
    def header(self, frame_index: bool = False) -> bytes:
        """Header text of ``write`` (Terse.hpp:454-470).  ``frame_index=True`` adds the ``frame_sizes`` and
        ``group_bit_offsets`` attributes: ignored by the reference reader, they let ``read``
        locate the frames and ``prolix`` expand them without any header walk."""
        h = _lib.trpx_header()
        h.prolix_bits, h.is_signed, h.block = self._prolix_bits, int(self._signed), self._block
        h.memory_size, h.number_of_values = len(self._data), self._size
        h.number_of_frames = self.number_of_frames()
        h.n_dims = len(self._dim)
        for i, d in enumerate(self._dim[:8]):
            h.dims[i] = d
        gs = None
        # (values of more than 32 bits -- 64-bit containers on the generic kernels -- have no decode index: frame sizes only)
        if frame_index and self._frame_sizes and self._prolix_bits <= 32 and lib().trpx_group_count(self._size, self._block):
            gs = self._states()
            if gs is None:                                   # compute them once: one walk of the stack on the device
                data = np.frombuffer(self._data, np.uint8)
                offs = np.concatenate([[0], np.cumsum(self._frame_sizes)]).astype(np.uint64)
                gs = np.zeros(lib().trpx_group_count(self._size, self._block) * len(self._frame_sizes), np.uint64)
                max_bits = 8 if self._prolix_bits <= 8 else 16 if self._prolix_bits <= 16 else 32
                rc = lib().trpx_group_states_host(data.ctypes.data, data.size, offs.ctypes.data, self._size, len(self._frame_sizes),
                                                  self._block, max_bits, gs.ctypes.data, self._device)
                del data
                if rc == 0:
                    self._group_states = gs
                elif rc == _lib.ERR_UNSUPPORTED:
                    gs = None                                # no group index for this stack: the file still gets its frame sizes
                else:
                    check(rc)                                # device fault, no device, corrupt stack: not "no index"
        cap = 512 + (21 * len(self._frame_sizes) + (16 * gs.size if gs is not None else 0) if frame_index else 0)
        buf = C.create_string_buffer(cap)
        if frame_index and gs is not None:
            sizes = np.asarray(self._frame_sizes, np.uint64)
            n = lib().trpx_header_format_grouped(C.byref(h), sizes.ctypes.data, sizes.size, gs.ctypes.data, gs.size, buf, cap)
        elif frame_index:
            sizes = np.asarray(self._frame_sizes, np.uint64)
            n = lib().trpx_header_format_indexed(C.byref(h), sizes.ctypes.data, sizes.size, buf, cap)
        else:
            n = lib().trpx_header_format(C.byref(h), buf, cap)
        if n == 0:
            raise RuntimeError("header does not fit")
        return buf.raw[:n]

    def write(self, ostream, frame_index: bool = False) -> None:
        ostream.write(self.header(frame_index))
        ostream.write(bytes(self._data))
        if hasattr(ostream, "flush"):
            ostream.flush()

    @classmethod
    def read(cls, istream, device: int = -1) -> "Terse":
        """``Terse(std::ifstream&)``: scan for the header, read the payload, leave the stream
        positioned on the byte after it (Terse.hpp:275-279)."""
        pos = istream.tell()
        h = _lib.trpx_header()
        off = C.c_size_t(0)
        want = 4096
        while True:                                          # an indexed header (frame_sizes) can be long: read more
            istream.seek(pos)
            blob = istream.read(want)
            rc = lib().trpx_header_parse(blob, len(blob), C.byref(h), C.byref(off))
            if rc == _lib.OK or len(blob) < want or want >= 1 << 28:
                break
            want <<= 4
        if rc != _lib.OK:
            raise ValueError("no valid <Terse .../> header found")   # the reference's stoul throws
        t = cls(block=h.block, device=device)
        t._prolix_bits, t._signed, t._size = h.prolix_bits, bool(h.is_signed), int(h.number_of_values)
        t._dim = [int(h.dims[i]) for i in range(h.n_dims)]
        istream.seek(pos + off.value)
        t._data = bytearray(istream.read(int(h.memory_size)))
        if len(t._data) != h.memory_size:
            raise ValueError("truncated .trpx payload")
        n_frames = int(h.number_of_frames)
        sizes = np.empty(max(n_frames, 1), np.uint64)
        have = lib().trpx_header_frame_sizes(blob, len(blob), sizes.ctypes.data, sizes.size)
        if n_frames == 1:
            t._frame_sizes = [len(t._data)]
        elif n_frames > 1 and have == n_frames and int(sizes.sum()) == len(t._data) and (sizes > 0).all():
            t._frame_sizes = [int(x) for x in sizes]          # row f1: the file carries its own frame index
        elif n_frames > 1:
            # The file stores no frame index: locate the frames with the device's header walk.
            buf = np.frombuffer(t._data, np.uint8)
            offs = np.empty(n_frames + 1, np.uint64)
            max_bits = 8 if h.prolix_bits <= 8 else 16 if h.prolix_bits <= 16 else 32
            check(lib().trpx_frame_offsets_host(buf.ctypes.data, buf.size, t._size, n_frames, t._block,
                                                max_bits, offs.ctypes.data, device))
            if int(offs[-1]) != len(t._data):
                raise ValueError("frame chain does not cover the payload (corrupt .trpx)")
            t._frame_sizes = [int(x) for x in np.diff(offs)]
        groups = lib().trpx_group_count(t._size, t._block) if t._size else 0
        if groups and t._frame_sizes:                        # row f1: group states, if the file has them (checked on the device when used)
            gs = np.zeros(groups * len(t._frame_sizes), np.uint64)
            if lib().trpx_header_group_states(blob, off.value, gs.ctypes.data, gs.size) == gs.size:
                t._group_states = gs
        return t
