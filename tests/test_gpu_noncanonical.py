"""GPU tests: every decoder on VALID streams that no encoder here writes -- restated and padded widths, the stream kinds of
tests/noncanonical.py (the reference decodes them all: tests/test_noncanonical_model.py, tests/golden/noncanonical.json).

Truth is the generator's pixels (numpy on them for sums, boxes and events), never anything the library returned.  Every
output lies between guard bands of 0x5A bytes and is itself filled with them; the status word is poisoned before each call.

The rules:
  1  floor, every cell: the outcome is EXACT (status 0, output bit-identical to truth) or REFUSED (TRPX_ERR_CORRUPT, as status
     or as a host call's return value), guards intact either way.  Status 0 with another output is a failure.
  2  exact is REQUIRED of every entry point on K0 and K2 (padded widths leave the layout rule alone), of trpx_locate_frames on
     every kind, and of trpx_decode_host, trpx_stack_read and Terse.prolix / prolix_stack on every kind.
  3  everything else on K1, K3, K4, K5 is pinned: PINNED holds the outcome observed on the MI355X per (cell, kind[, shape]).
     A later change from exact to refused, or back, fails until someone edits the table on purpose.
  4  one graph capture of trpx_decode on a K1 stack, replayed onto a K0 stack of the same geometry and back.

A cell is "entry|input form|route"."""
import ctypes as C
import io

import numpy as np
import pytest

import noncanonical as nc
from gpu_support import sparse_truth, to_dev

pytestmark = pytest.mark.gpu

GB = 512                      # guard band, bytes: 64 elements of the widest type
FILL = 0x5A
OK, CORRUPT = 0, 5
EXACT, REFUSED = "exact", "refused"
ROUTES = (0, 1, 2, 3, 4, 5)

SHAPES = [(3, 7000), (4, 1073), (2, 7), (2, 3073), (130, 388), (3, 12 * 34000 + 3), (2, 1030 * 1065)]
FULL_SHAPES = SHAPES[:2]                                     # the full type list, on K0 .. K3


def _cases():
    out = []
    for shape in SHAPES:
        for kind in nc.KINDS:
            full = shape in FULL_SHAPES and kind in ("K0", "K1", "K2", "K3")
            for dt in (nc.ALL_DTYPES if full else [np.uint16, np.int32]):
                out.append(pytest.param(shape, kind, dt, id=f"{shape[0]}x{shape[1]}-{kind}-{np.dtype(dt).name}"))
    return out


def n_variants(shape, kind, dt):
    """K4: every (placement, run width) pair on the small shapes, four variants of the large ones."""
    v = nc.variants(shape, kind, dt)
    return v if shape[1] <= 7000 else min(v, 4)


# ---- the pinned outcomes (rule 3) --------------------------------------------------------------------------------------------
# Observed on the MI355X, as (cells, {kind: outcome | {shape: outcome | {pixel type: outcome}}}).  In words:
# the basic route, the converting decode, trpx_decode without offsets on stacks too small for the parallel locator (the basic
# kernels) and trpx_decode_host_grouped decode restated widths; trpx_build_index refuses them, and with it everything that
# builds its index on the way (sum, roi, sparse without an index, and their host forms); an index, once built, is good (the
# 2 x 7 stacks, whose one-block frames restate nothing); on trpx_decode's other routes a frame the per-frame decoder extracts from its own walk
# is exact, and a frame that goes through widths -- header-dense, more than 32 K blocks, the tiled route -- is refused.
_PINNED_GROUPS = [(['build_index|offsets|0', 'roi_host|offsets|0', 'roi|none|0', 'roi|offsets|0', 'sparse_host|offsets|0', 'sparse|none|0',
   'sparse|offsets|0', 'sum_host|offsets|0', 'sum|none|0', 'sum|offsets|0'],
  {'K1': {'130x388': 'refused',
          '2x1096950': 'refused',
          '2x3073': 'refused',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': 'refused',
          '4x1073': 'refused'},
   'K3': {'130x388': 'refused',
          '2x1096950': 'refused',
          '2x3073': 'refused',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': 'refused',
          '4x1073': 'refused'},
   'K4': 'refused',
   'K5': 'refused'}),
 (['convert|none|0', 'convert|offsets|0', 'decode|none|0', 'decode|none|1', 'decode|none|3', 'decode|none|4', 'decode|none|5',
   'decode|offsets|1', 'host_grouped|offsets|0'],
  {'K1': 'exact', 'K3': 'exact', 'K4': 'exact', 'K5': 'exact'}),
 (['decode|none|2'],
  {'K1': {'130x388': 'refused',
          '2x1096950': 'exact',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'exact',
          '3x7000': 'exact',
          '4x1073': 'exact'},
   'K3': {'130x388': 'refused',
          '2x1096950': 'exact',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'exact',
          '3x7000': 'exact',
          '4x1073': 'exact'},
   'K4': {'130x388': 'refused',
          '2x1096950': 'exact',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'exact',
          '3x7000': 'exact',
          '4x1073': 'exact'},
   'K5': {'130x388': 'refused',
          '2x1096950': 'exact',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'exact',
          '3x7000': 'exact',
          '4x1073': 'exact'}}),
 (['decode|offsets|0', 'decode|offsets|3', 'decode|offsets|5'],
  {'K1': {'130x388': 'exact',
          '2x1096950': 'refused',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': {'int16': 'exact',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'exact',
                     'uint16': 'exact',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'exact'},
          '4x1073': 'exact'},
   'K3': {'130x388': 'exact',
          '2x1096950': 'refused',
          '2x3073': 'refused',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': {'int16': 'refused',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'refused',
                     'uint16': 'refused',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'refused'},
          '4x1073': 'exact'},
   'K4': {'130x388': 'exact',
          '2x1096950': {'int32': 'refused', 'uint16': 'exact'},
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': {'int32': 'refused', 'uint16': 'exact'},
          '3x7000': 'exact',
          '4x1073': 'exact'},
   'K5': {'130x388': 'exact',
          '2x1096950': 'refused',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': 'exact',
          '4x1073': 'exact'}}),
 (['decode|offsets|2'],
  {'K1': {'130x388': 'refused',
          '2x1096950': 'refused',
          '2x3073': 'refused',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': {'int16': 'refused',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'refused',
                     'uint16': 'refused',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'refused'},
          '4x1073': {'int16': 'refused',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'refused',
                     'uint16': 'refused',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'refused'}},
   'K3': {'130x388': 'refused',
          '2x1096950': 'refused',
          '2x3073': 'refused',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': {'int16': 'refused',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'refused',
                     'uint16': 'refused',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'refused'},
          '4x1073': {'int16': 'refused',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'refused',
                     'uint16': 'refused',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'refused'}},
   'K4': 'refused',
   'K5': 'refused'}),
 (['decode|offsets|4'],
  {'K1': {'130x388': 'exact',
          '2x1096950': 'refused',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': {'int16': 'exact',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'exact',
                     'uint16': 'exact',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'exact'},
          '4x1073': 'exact'},
   'K3': {'130x388': 'exact',
          '2x1096950': 'refused',
          '2x3073': 'refused',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': {'int16': 'refused',
                     'int32': 'refused',
                     'int64': 'exact',
                     'int8': 'refused',
                     'uint16': 'refused',
                     'uint32': 'refused',
                     'uint64': 'exact',
                     'uint8': 'refused'},
          '4x1073': 'exact'},
   'K4': 'exact',
   'K5': {'130x388': 'exact',
          '2x1096950': 'refused',
          '2x3073': 'exact',
          '2x7': 'exact',
          '3x408003': 'refused',
          '3x7000': 'exact',
          '4x1073': 'exact'}}),
 (['indexed|index|0', 'indexed|index|2', 'indexed|index|3', 'roi|index|0', 'sparse|index|0', 'states|index|0', 'sum|index|0'],
  {'K1': 'exact', 'K3': 'exact'})]
PINNED = {cell: tab for cells, tab in _PINNED_GROUPS for cell in cells}


def pinned(cell, kind, shape, dt):
    v = PINNED[cell][kind]
    if isinstance(v, dict):
        v = v[f"{shape[0]}x{shape[1]}"]
    if isinstance(v, dict):
        v = v[np.dtype(dt).name]
    return v


def required_exact(cell, kind):
    entry = cell.split("|")[0]
    return kind in ("K0", "K2") or entry in ("locate", "host_decode", "stack_read", "prolix", "prolix_stack")


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def _L():
    import torch  # noqa: F401  (before the library, as the gpu fixture does: one HIP runtime in the process)
    from trpx_amd import _lib
    return _lib.lib()


def _code(dt):
    from trpx_amd import terse
    return terse._code(dt, True)


def _stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _buf(nbytes):
    import torch
    return torch.full((nbytes + 2 * GB,), FILL, dtype=torch.uint8, device="cuda")


def _ptr(t):
    return t.data_ptr() + GB


def _read(t, nbytes):
    a = t.cpu().numpy()
    return a[GB: GB + nbytes], bool((a[:GB] == FILL).all() and (a[GB + nbytes:] == FILL).all())


def _status():
    import torch
    return torch.full((8,), 77, dtype=torch.int32, device="cuda")


def _verdict(rc, status, outs):
    """outs: (bytes got, guards intact, bytes wanted) per output array"""
    if rc:
        return f"WRONG: return code {rc}"
    if not all(g for _, g, _ in outs):
        return "WRONG: written outside an output"
    if status == OK:
        return EXACT if all(np.array_equal(a, np.ascontiguousarray(w).view(np.uint8).reshape(-1)) for a, _, w in outs) else "WRONG: status 0, wrong output"
    return REFUSED if status == CORRUPT else f"WRONG: status {status}"


def _host_verdict(rc, outs):
    if rc == CORRUPT:
        return REFUSED if all(g for _, g, _ in outs) else "WRONG: written outside an output"
    return _verdict(rc, OK, outs) if rc == OK else f"WRONG: return code {rc}"


def _hbuf(nbytes):
    return np.full(nbytes + 2 * GB, FILL, np.uint8)


def _hread(a, nbytes):
    return a[GB: GB + nbytes], bool((a[:GB] == FILL).all() and (a[GB + nbytes:] == FILL).all())


class Dev:
    """One stack on the device, and the calls on it."""

    def __init__(self, S, pad_to=0):
        import torch
        self.S, self.dt = S, S.dt
        self.frames, self.n = S.shape
        self.nbytes = max(S.stream.size, pad_to)
        host = np.zeros(self.nbytes + 16, np.uint8)
        host[: S.stream.size] = S.stream
        self.terse = torch.from_numpy(host).cuda()
        self.offs = torch.from_numpy(S.offsets.astype(np.int64)).cuda()
        self.code = _code(S.dt)
        self.signed = int(S.dt.kind == "i")
        self.tuned = S.dt.itemsize < 8

    def _sync(self, st):
        import torch
        torch.cuda.synchronize()
        return int(st[0].item())

    def _ws(self, nbytes):
        import torch
        return torch.empty(max(int(nbytes), 256) + 256, dtype=torch.uint8, device="cuda")

    def decode(self, form, out_dt=None, convert=False):
        L = _L()
        odt = np.dtype(out_dt or self.dt)
        want = self.S.px.astype(odt)
        out, st = _buf(want.nbytes), _status()
        ws = self._ws(max(L.trpx_decode_workspace_bytes(c, self.n, self.frames, 12) for c in (0, 5, _code(odt))))
        fn = L.trpx_decode_convert if convert else L.trpx_decode
        rc = fn(self.signed, _code(odt), self.terse.data_ptr(), self.nbytes, self.offs.data_ptr() if form == "offsets" else None,
                self.n, self.frames, 12, _ptr(out), st.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        status = self._sync(st)
        return _verdict(rc, status, [_read(out, want.nbytes) + (want,)])

    def locate(self):
        L = _L()
        want = self.S.offsets.astype(np.int64)
        out, st = _buf(want.nbytes), _status()
        ws = self._ws(L.trpx_locate_workspace_bytes(self.nbytes, self.n, self.frames, 12))
        # (the stack's true size: the locator checks that the frames cover it)
        rc = L.trpx_locate_frames(self.terse.data_ptr(), self.S.stream.size, self.n, self.frames, 12, 8 * self.dt.itemsize, _ptr(out),
                                  st.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        status = self._sync(st)
        return _verdict(rc, status, [_read(out, want.nbytes) + (want,)])

    def build_index(self):
        L = _L()
        nb = L.trpx_index_bytes(self.code, self.n, self.frames, 12)
        idx, st = _buf(nb), _status()
        rc = L.trpx_build_index(self.code, self.terse.data_ptr(), self.nbytes, self.offs.data_ptr(), self.n, self.frames, 12, _ptr(idx),
                                st.data_ptr(), _stream_ptr())
        status = self._sync(st)
        a = idx.cpu().numpy()
        guards = bool((a[:GB] == FILL).all() and (a[GB + nb:] == FILL).all())
        v = _verdict(rc, status, [(None, guards, None)]) if (rc or not guards or status != OK) else EXACT
        return v, (idx if v == EXACT else None), nb

    def indexed(self, idx):
        L = _L()
        want = self.S.px
        out, st = _buf(want.nbytes), _status()
        rc = L.trpx_decode_indexed(self.signed, self.code, self.terse.data_ptr(), self.nbytes, self.offs.data_ptr(), _ptr(idx), self.n,
                                   self.frames, 12, _ptr(out), st.data_ptr(), _stream_ptr())
        status = self._sync(st)
        return _verdict(rc, status, [_read(out, want.nbytes) + (want,)])

    def via_states(self, idx, nb):
        import torch
        L = _L()
        ng = L.trpx_group_count(self.n, 12) * self.frames
        states = torch.zeros(ng, dtype=torch.int64, device="cuda")
        rc = L.trpx_index_group_states(_ptr(idx), self.n, self.frames, 12, states.data_ptr(), _stream_ptr())
        if rc:
            return f"WRONG: return code {rc}"
        rebuilt, st = _buf(nb), _status()
        rc = L.trpx_index_from_group_states(self.code, self.terse.data_ptr(), self.nbytes, self.offs.data_ptr(), states.data_ptr(), self.n,
                                            self.frames, 12, _ptr(rebuilt), st.data_ptr(), _stream_ptr())
        status = self._sync(st)
        a = rebuilt.cpu().numpy()
        if rc or status not in (OK, CORRUPT) or not ((a[:GB] == FILL).all() and (a[GB + nb:] == FILL).all()):
            return f"WRONG: index from group states: rc {rc}, status {status}, or written outside the index"
        return REFUSED if status == CORRUPT else self.indexed(rebuilt)

    def _forms(self, form, idx):
        return (self.offs.data_ptr() if form != "none" else None), (_ptr(idx) if form == "index" else None)

    def sum(self, form, idx, group):
        L = _L()
        f, n = self.frames, self.n
        px = self.S.px.astype(np.int64)
        want = np.stack([px[g: g + group].sum(axis=0) for g in range(0, f, group)])
        out, st = _buf(want.nbytes), _status()
        ws = self._ws(L.trpx_decode_sum_workspace_bytes(self.code, self.nbytes, n, f, 12, group))
        offs, index = self._forms(form, idx)
        rc = L.trpx_decode_sum(self.code, _code(np.int64), self.terse.data_ptr(), self.nbytes, offs, index, n, f, 12, group, _ptr(out),
                               st.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        status = self._sync(st)
        return _verdict(rc, status, [_read(out, want.nbytes) + (want,)])

    def boxes(self, which):
        """(boxes uint32 [k, 3], h, w, truth): the frame as one row of n pixels"""
        f, n = self.frames, self.n
        if which == "whole":
            w, x0 = n, 0
        else:                                                # inside the frame's last group of 256 blocks
            g0 = (-(-n // 12) - 1) // 256 * 256 * 12
            w = min(40, n - g0)
            x0 = n - w
        b = np.array([(k, 0, x0) for k in range(f)], np.uint32)
        return b, 1, w, np.ascontiguousarray(self.S.px[:, x0: x0 + w])

    def roi(self, form, idx, which):
        L = _L()
        b, h, w, want = self.boxes(which)
        out, st = _buf(want.nbytes), _status()
        ws = self._ws(L.trpx_decode_roi_workspace_bytes(self.code, self.nbytes, self.n, self.frames, 12))
        db = to_dev(b)
        offs, index = self._forms(form, idx)
        rc = L.trpx_decode_roi(self.code, self.terse.data_ptr(), self.nbytes, offs, index, self.n, self.frames, 12, self.n, db.data_ptr(),
                               b.shape[0], h, w, _ptr(out), st.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        status = self._sync(st)
        return _verdict(rc, status, [_read(out, want.nbytes) + (want,)])

    def sparse(self, form, idx, t):
        L = _L()
        rows, pos, val = sparse_truth(self.S.px, t)
        total = int(rows[-1])
        r, p, v, st = _buf(rows.nbytes), _buf(pos.nbytes), _buf(val.nbytes), _status()
        ws = self._ws(L.trpx_decode_sparse_workspace_bytes(self.code, self.nbytes, self.n, self.frames, 12))
        offs, index = self._forms(form, idx)
        rc = L.trpx_decode_sparse(self.code, self.terse.data_ptr(), self.nbytes, offs, index, self.n, self.frames, 12, int(t), _ptr(r),
                                  _ptr(p) if total else None, _ptr(v) if total else None, total, st.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream_ptr())
        status = self._sync(st)
        return _verdict(rc, status, [_read(r, rows.nbytes) + (rows,), _read(p, pos.nbytes) + (pos,), _read(v, val.nbytes) + (val,)])


# ---- host entry points ---------------------------------------------------------------------------------------------------------
def _host_cells(S, D):
    from trpx_amd import _lib, terse
    L = _L()
    frames, n = S.shape
    buf = np.ascontiguousarray(S.stream)
    offs = S.offsets.astype(np.uint64)
    code, signed = _code(S.dt), int(S.dt.kind == "i")
    cells = {}
    for form in ("offsets", "none"):
        out = _hbuf(S.px.nbytes)
        rc = L.trpx_decode_host(signed, code, buf.ctypes.data, buf.size, offs.ctypes.data if form == "offsets" else None, n, frames, 12,
                                out.ctypes.data + GB, -1)
        cells[f"host_decode|{form}|0"] = _host_verdict(rc, [_hread(out, S.px.nbytes) + (S.px,)])
    out = _hbuf(S.px.nbytes)
    rc = L.trpx_decode_host_grouped(signed, code, buf.ctypes.data, buf.size, offs.ctypes.data, None, n, frames, 12, out.ctypes.data + GB, -1)
    cells["host_grouped|offsets|0"] = _host_verdict(rc, [_hread(out, S.px.nbytes) + (S.px,)])
    # trpx_stack_open / trpx_stack_read, frame by frame
    h = C.c_void_p()
    rc = L.trpx_stack_open(C.byref(h), signed, buf.ctypes.data, buf.size, offs.ctypes.data, None, n, frames, 12, 0, -1)
    if rc:
        cells["stack_read|offsets|0"] = REFUSED if rc == CORRUPT else f"WRONG: trpx_stack_open returns {rc}"
    else:
        try:
            vs = set()
            for f in range(frames):
                out = _hbuf(S.px[f].nbytes)
                rc = L.trpx_stack_read(h, f, code, out.ctypes.data + GB)
                vs.add(_host_verdict(rc, [_hread(out, S.px[f].nbytes) + (S.px[f],)]))
            cells["stack_read|offsets|0"] = vs.pop() if len(vs) == 1 else "WRONG: " + " / ".join(sorted(vs))
        finally:
            L.trpx_stack_close(h)
    # Terse.prolix / prolix_stack on a file written with the test's stream (no frame index in it: read() locates the frames)
    t = terse.Terse()
    t._signed, t._size, t._prolix_bits = bool(signed), n, S.prolix_bits
    t._data = bytearray(S.stream.tobytes())
    t._frame_sizes = [int(x) for x in np.diff(S.offsets)]
    f = io.BytesIO()
    t.write(f)
    f.seek(0)
    try:
        r = terse.Terse.read(f)
        assert r.frame_sizes() == t._frame_sizes and r.size() == n and r.number_of_frames() == frames
        vs = set()
        for k in range(frames):
            out = np.full(n, FILL, S.dt)
            r.prolix(out, k)
            vs.add(EXACT if out.tobytes() == S.px[k].tobytes() else "WRONG: status 0, wrong output")
        cells["prolix|file|0"] = vs.pop() if len(vs) == 1 else "WRONG: " + " / ".join(sorted(vs))
        back = r.prolix_stack(S.dt)
        cells["prolix_stack|file|0"] = EXACT if back.tobytes() == S.px.tobytes() else "WRONG: status 0, wrong output"
    except _lib.TrpxError as e:
        for c in ("prolix|file|0", "prolix_stack|file|0"):
            cells.setdefault(c, REFUSED if e.code == CORRUPT else f"WRONG: {e}")
    if not D.tuned:
        return cells
    px = S.px.astype(np.int64)
    for name, group in (("sum1", 1), ("sumall", frames)):
        want = np.stack([px[g: g + group].sum(axis=0) for g in range(0, frames, group)])
        out = _hbuf(want.nbytes)
        rc = L.trpx_decode_sum_host(code, _code(np.int64), buf.ctypes.data, buf.size, offs.ctypes.data, n, frames, 12, group, out.ctypes.data + GB, -1)
        cells[f"sum_host|offsets|0:{name}"] = _host_verdict(rc, [_hread(out, want.nbytes) + (want,)])
    for which in ("whole", "last"):
        b, h_, w_, want = D.boxes(which)
        out = _hbuf(want.nbytes)
        rc = L.trpx_decode_roi_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, n, frames, 12, n, b.ctypes.data, b.shape[0], h_, w_,
                                    out.ctypes.data + GB, -1)
        cells[f"roi_host|offsets|0:{which}"] = _host_verdict(rc, [_hread(out, want.nbytes) + (want,)])
    for thr in (1, 1 << 7):
        rows, pos, val = sparse_truth(S.px, thr)
        total = int(rows[-1])
        r_, p_, v_ = _hbuf(rows.nbytes), _hbuf(pos.nbytes), _hbuf(val.nbytes)
        found = C.c_size_t(0)
        rc = L.trpx_decode_sparse_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, n, frames, 12, thr, r_.ctypes.data + GB,
                                       p_.ctypes.data + GB if total else None, v_.ctypes.data + GB if total else None, total, C.byref(found), -1)
        cells[f"sparse_host|offsets|0:{thr}"] = _host_verdict(rc, [_hread(r_, rows.nbytes) + (rows,), _hread(p_, pos.nbytes) + (pos,),
                                                                   _hread(v_, val.nbytes) + (val,)])
    return cells


def _merge(cells):
    """sub-cells "cell:what" -> one verdict per cell: the common one, else all of them"""
    out = {}
    for k, v in cells.items():
        out.setdefault(k.split(":")[0], set()).add(v)
    return {k: (vs.pop() if len(vs) == 1 else ("WRONG: " if any(x.startswith("WRONG") for x in vs) else "mixed: ") + " / ".join(sorted(vs)))
            for k, vs in out.items()}


def run_stack(S):
    """Every cell on one stack: {cell: verdict}"""
    L = _L()
    D = Dev(S)
    cells = {}
    try:
        for route in ROUTES:
            assert L.trpx_set_decode_path(route) == 0
            for form in ("offsets", "none"):
                cells[f"decode|{form}|{route}"] = D.decode(form)
    finally:
        L.trpx_set_decode_path(0)
    conv = {np.dtype(np.uint16): np.float32, np.dtype(np.int32): np.int64}.get(S.dt)
    if conv:
        for form in ("offsets", "none"):
            cells[f"convert|{form}|0"] = D.decode(form, conv, convert=True)
    try:
        for path in (0, 1):
            assert L.trpx_set_locate_path(path) == 0
            cells[f"locate|none|{path}"] = D.locate()
    finally:
        L.trpx_set_locate_path(0)
    if D.tuned:
        v, idx, nb = D.build_index()
        cells["build_index|offsets|0"] = v
        if idx is not None:
            try:
                for route in (0, 2, 3):
                    assert L.trpx_set_decode_path(route) == 0
                    cells[f"indexed|index|{route}"] = D.indexed(idx)
            finally:
                L.trpx_set_decode_path(0)
            cells["states|index|0"] = D.via_states(idx, nb)
        for form in ("index", "offsets", "none"):
            if form == "index" and idx is None:
                continue
            cells[f"sum|{form}|0:1"] = D.sum(form, idx, 1)
            cells[f"sum|{form}|0:all"] = D.sum(form, idx, D.frames)
            cells[f"roi|{form}|0:whole"] = D.roi(form, idx, "whole")
            cells[f"roi|{form}|0:last"] = D.roi(form, idx, "last")
            cells[f"sparse|{form}|0:1"] = D.sparse(form, idx, 1)
            cells[f"sparse|{form}|0:128"] = D.sparse(form, idx, 1 << 7)
    cells.update(_host_cells(S, D))
    return _merge(cells)


def run_case(shape, kind, dt):
    """Every cell over the case's variants: {cell: verdict} (one verdict where the variants agree)"""
    per = [run_stack(nc.make(dt, shape, kind, v)) for v in range(n_variants(shape, kind, dt))]
    out = {}
    for cell in per[0]:
        vs = {p.get(cell, "absent") for p in per}
        out[cell] = vs.pop() if len(vs) == 1 else ("WRONG: " if any(x.startswith("WRONG") for x in vs) else "mixed: ") + " / ".join(sorted(vs))
    return out


def judge(shape, kind, dt, cells):
    """The failures of one case against rules 1 - 3"""
    bad = []
    for cell, v in sorted(cells.items()):
        if v not in (EXACT, REFUSED):
            bad.append(f"rule 1: {cell}: {v}")
        elif required_exact(cell, kind):
            if v != EXACT:
                bad.append(f"rule 2: {cell}: {v}, exact is required")
        elif v != pinned(cell, kind, shape, dt):
            bad.append(f"rule 3: {cell}: {v}, pinned {pinned(cell, kind, shape, dt)}")
    return bad


@pytest.mark.parametrize("shape,kind,dt", _cases())
def test_every_decoder(gpu, shape, kind, dt):
    cells = run_case(shape, kind, dt)
    assert len(cells) >= (30 if np.dtype(dt).itemsize < 8 else 18), sorted(cells)     # (30: no index, no converting pair)
    bad = judge(shape, kind, dt, cells)
    assert not bad, "\n".join([f"{shape} {kind} {np.dtype(dt).name}:"] + bad)


def test_graph_capture_replays_across_kinds(gpu):
    """Rule 4: trpx_decode captured on a K1 stack, replayed onto a K0 stack of the same geometry and back: each replay gives
    the outcome pinned for its kind (nothing of the first stream's layout stays in the graph or the workspace)."""
    import torch
    L = _L()
    shape, dt = (3, 7000), np.dtype(np.uint16)
    k1, k0 = nc.make(dt, shape, "K1"), nc.make(dt, shape, "K0")
    assert k1.stream.size != k0.stream.size
    cap = max(k1.stream.size, k0.stream.size)
    terse = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(shape[0] + 1, dtype=torch.int64, device="cuda")
    nbytes = k1.px.nbytes
    out, st = _buf(nbytes), _status()
    ws = torch.empty(L.trpx_decode_workspace_bytes(_code(dt), shape[1], shape[0], 12) + 256, dtype=torch.uint8, device="cuda")

    def load(S):
        host = np.zeros(cap + 16, np.uint8)
        host[: S.stream.size] = S.stream
        terse.copy_(torch.from_numpy(host))
        offs.copy_(torch.from_numpy(S.offsets.astype(np.int64)))
        out.fill_(FILL)
        st.fill_(77)

    def call():
        return L.trpx_decode(0, _code(dt), terse.data_ptr(), cap, offs.data_ptr(), shape[1], shape[0], 12, _ptr(out), st.data_ptr(),
                             ws.data_ptr(), ws.numel(), _stream_ptr())

    load(k1)
    assert call() == 0                                      # (eager warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert call() == 0
    for S in (k1, k0, k1, k0):
        load(S)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        v = _verdict(0, int(st[0].item()), [_read(out, nbytes) + (S.px,)])
        want = EXACT if S.kind == "K0" else pinned("decode|offsets|0", S.kind, shape, dt)
        assert v == want, (S.kind, v, want)
