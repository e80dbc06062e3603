"""The device side of the tests on valid streams that no encoder here writes (tests/noncanonical.py makes the streams):
a stack on the device with every decoding call on it (Dev), the guarded buffers and the verdict of a call, and the outcomes
pinned per cell (PINNED, pinned(), required_exact(); the rules are in tests/test_gpu_noncanonical.py and DESIGN.md section 4.13).
Not a test module: tests/test_gpu_noncanonical.py and the route tests of tests/test_gpu_parity.py import it.

Every output lies between guard bands of 0x5A bytes and is itself filled with them; the status word is poisoned before each
call.  A verdict is EXACT (status 0, output bit-identical to truth), REFUSED (TRPX_ERR_CORRUPT, guards intact) or a string
that starts with "WRONG"."""
import numpy as np

from gpu_support import CORRUPT, OK, sparse_truth, status_block, to_dev

GB = 512                      # guard band, bytes: 64 elements of the widest type
FILL = 0x5A
EXACT, REFUSED = "exact", "refused"


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
def lib():
    import torch  # noqa: F401  (before the library, as the gpu fixture does: one HIP runtime in the process)
    from trpx_amd import _lib
    return _lib.lib()


def code_of(dt):
    from trpx_amd import terse
    return terse._code(dt, True)


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def dev_buf(nbytes):
    import torch
    return torch.full((nbytes + 2 * GB,), FILL, dtype=torch.uint8, device="cuda")


def inner_ptr(t):
    return t.data_ptr() + GB


def dev_read(t, nbytes):
    a = t.cpu().numpy()
    return a[GB: GB + nbytes], bool((a[:GB] == FILL).all() and (a[GB + nbytes:] == FILL).all())


def verdict(rc, status, outs):
    """outs: (bytes got, guards intact, bytes wanted) per output array"""
    if rc:
        return f"WRONG: return code {rc}"
    if not all(g for _, g, _ in outs):
        return "WRONG: written outside an output"
    if status == OK:
        return EXACT if all(np.array_equal(a, np.ascontiguousarray(w).view(np.uint8).reshape(-1)) for a, _, w in outs) else "WRONG: status 0, wrong output"
    return REFUSED if status == CORRUPT else f"WRONG: status {status}"


def host_verdict(rc, outs):
    if rc == CORRUPT:
        return REFUSED if all(g for _, g, _ in outs) else "WRONG: written outside an output"
    return verdict(rc, OK, outs) if rc == OK else f"WRONG: return code {rc}"


def host_buf(nbytes):
    return np.full(nbytes + 2 * GB, FILL, np.uint8)


def host_read(a, nbytes):
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
        self.code = code_of(S.dt)
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
        L = lib()
        odt = np.dtype(out_dt or self.dt)
        want = self.S.px.astype(odt)
        out, st = dev_buf(want.nbytes), status_block()
        ws = self._ws(max(L.trpx_decode_workspace_bytes(c, self.n, self.frames, 12) for c in (0, 5, code_of(odt))))
        fn = L.trpx_decode_convert if convert else L.trpx_decode
        rc = fn(self.signed, code_of(odt), self.terse.data_ptr(), self.nbytes, self.offs.data_ptr() if form == "offsets" else None,
                self.n, self.frames, 12, inner_ptr(out), st.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
        status = self._sync(st)
        return verdict(rc, status, [dev_read(out, want.nbytes) + (want,)])

    def locate(self):
        L = lib()
        want = self.S.offsets.astype(np.int64)
        out, st = dev_buf(want.nbytes), status_block()
        ws = self._ws(L.trpx_locate_workspace_bytes(self.nbytes, self.n, self.frames, 12))
        # (the stack's true size: the locator checks that the frames cover it)
        rc = L.trpx_locate_frames(self.terse.data_ptr(), self.S.stream.size, self.n, self.frames, 12, 8 * self.dt.itemsize, inner_ptr(out),
                                  st.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
        status = self._sync(st)
        return verdict(rc, status, [dev_read(out, want.nbytes) + (want,)])

    def build_index(self):
        L = lib()
        nb = L.trpx_index_bytes(self.code, self.n, self.frames, 12)
        idx, st = dev_buf(nb), status_block()
        rc = L.trpx_build_index(self.code, self.terse.data_ptr(), self.nbytes, self.offs.data_ptr(), self.n, self.frames, 12, inner_ptr(idx),
                                st.data_ptr(), stream_ptr())
        status = self._sync(st)
        a = idx.cpu().numpy()
        guards = bool((a[:GB] == FILL).all() and (a[GB + nb:] == FILL).all())
        v = verdict(rc, status, [(None, guards, None)]) if (rc or not guards or status != OK) else EXACT
        return v, (idx if v == EXACT else None), nb

    def indexed(self, idx):
        L = lib()
        want = self.S.px
        out, st = dev_buf(want.nbytes), status_block()
        rc = L.trpx_decode_indexed(self.signed, self.code, self.terse.data_ptr(), self.nbytes, self.offs.data_ptr(), inner_ptr(idx), self.n,
                                   self.frames, 12, inner_ptr(out), st.data_ptr(), stream_ptr())
        status = self._sync(st)
        return verdict(rc, status, [dev_read(out, want.nbytes) + (want,)])

    def via_states(self, idx, nb):
        import torch
        L = lib()
        ng = L.trpx_group_count(self.n, 12) * self.frames
        states = torch.zeros(ng, dtype=torch.int64, device="cuda")
        rc = L.trpx_index_group_states(inner_ptr(idx), self.n, self.frames, 12, states.data_ptr(), stream_ptr())
        if rc:
            return f"WRONG: return code {rc}"
        rebuilt, st = dev_buf(nb), status_block()
        rc = L.trpx_index_from_group_states(self.code, self.terse.data_ptr(), self.nbytes, self.offs.data_ptr(), states.data_ptr(), self.n,
                                            self.frames, 12, inner_ptr(rebuilt), st.data_ptr(), stream_ptr())
        status = self._sync(st)
        a = rebuilt.cpu().numpy()
        if rc or status not in (OK, CORRUPT) or not ((a[:GB] == FILL).all() and (a[GB + nb:] == FILL).all()):
            return f"WRONG: index from group states: rc {rc}, status {status}, or written outside the index"
        return REFUSED if status == CORRUPT else self.indexed(rebuilt)

    def _forms(self, form, idx):
        return (self.offs.data_ptr() if form != "none" else None), (inner_ptr(idx) if form == "index" else None)

    def sum(self, form, idx, group):
        L = lib()
        f, n = self.frames, self.n
        px = self.S.px.astype(np.int64)
        want = np.stack([px[g: g + group].sum(axis=0) for g in range(0, f, group)])
        out, st = dev_buf(want.nbytes), status_block()
        ws = self._ws(L.trpx_decode_sum_workspace_bytes(self.code, self.nbytes, n, f, 12, group))
        offs, index = self._forms(form, idx)
        rc = L.trpx_decode_sum(self.code, code_of(np.int64), self.terse.data_ptr(), self.nbytes, offs, index, n, f, 12, group, inner_ptr(out),
                               st.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
        status = self._sync(st)
        return verdict(rc, status, [dev_read(out, want.nbytes) + (want,)])

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
        L = lib()
        b, h, w, want = self.boxes(which)
        out, st = dev_buf(want.nbytes), status_block()
        ws = self._ws(L.trpx_decode_roi_workspace_bytes(self.code, self.nbytes, self.n, self.frames, 12))
        db = to_dev(b)
        offs, index = self._forms(form, idx)
        rc = L.trpx_decode_roi(self.code, self.terse.data_ptr(), self.nbytes, offs, index, self.n, self.frames, 12, self.n, db.data_ptr(),
                               b.shape[0], h, w, inner_ptr(out), st.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
        status = self._sync(st)
        return verdict(rc, status, [dev_read(out, want.nbytes) + (want,)])

    def sparse(self, form, idx, t):
        L = lib()
        rows, pos, val = sparse_truth(self.S.px, t)
        total = int(rows[-1])
        r, p, v, st = dev_buf(rows.nbytes), dev_buf(pos.nbytes), dev_buf(val.nbytes), status_block()
        ws = self._ws(L.trpx_decode_sparse_workspace_bytes(self.code, self.nbytes, self.n, self.frames, 12))
        offs, index = self._forms(form, idx)
        rc = L.trpx_decode_sparse(self.code, self.terse.data_ptr(), self.nbytes, offs, index, self.n, self.frames, 12, int(t), inner_ptr(r),
                                  inner_ptr(p) if total else None, inner_ptr(v) if total else None, total, st.data_ptr(), ws.data_ptr(), ws.numel(),
                                  stream_ptr())
        status = self._sync(st)
        return verdict(rc, status, [dev_read(r, rows.nbytes) + (rows,), dev_read(p, pos.nbytes) + (pos,), dev_read(v, val.nbytes) + (val,)])
