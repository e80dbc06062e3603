"""GPU tests: every decoder on VALID streams that no encoder here writes -- restated and padded widths, the stream kinds of
tests/noncanonical.py (the reference decodes them all: tests/test_noncanonical_model.py, tests/golden/noncanonical.json).

Truth is the generator's pixels (numpy on them for sums, boxes and events), never anything the library returned.  Every
output lies between guard bands of 0x5A bytes and is itself filled with them; the status word is poisoned before each call.

The rules:
  1  floor, every cell: the outcome is EXACT (status 0, output bit-identical to truth) or REFUSED (TRPX_ERR_CORRUPT, as status
     or as a host call's return value), guards intact either way.  Status 0 with another output is a failure.
  2  exact is REQUIRED of every entry point on K0 and K2 (padded widths leave the layout rule alone), of trpx_locate_frames on
     every kind, and of trpx_decode_host, trpx_stack_read and Terse.prolix / prolix_stack on every kind.
  3  everything else on K1, K3, K4, K5 is pinned: PINNED (tests/noncanonical_dev.py) holds the outcome observed on the MI355X per (cell, kind[, shape]).
     A later change from exact to refused, or back, fails until someone edits the table on purpose.
  4  one graph capture of trpx_decode on a K1 stack, replayed onto a K0 stack of the same geometry and back.

A cell is "entry|input form|route"."""
import ctypes as C
import io

import numpy as np
import pytest

import noncanonical as nc
from gpu_support import CORRUPT, selected, sparse_truth, status_block
from noncanonical_dev import (EXACT, FILL, GB, REFUSED, Dev, code_of, dev_buf, dev_read, host_buf, host_read, host_verdict, inner_ptr,
                              lib, pinned, required_exact, stream_ptr, verdict)

pytestmark = pytest.mark.gpu

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


# ---- host entry points ---------------------------------------------------------------------------------------------------------
def _host_cells(S, D):
    from trpx_amd import _lib, terse
    L = lib()
    frames, n = S.shape
    buf = np.ascontiguousarray(S.stream)
    offs = S.offsets.astype(np.uint64)
    code, signed = code_of(S.dt), int(S.dt.kind == "i")
    cells = {}
    for form in ("offsets", "none"):
        out = host_buf(S.px.nbytes)
        rc = L.trpx_decode_host(signed, code, buf.ctypes.data, buf.size, offs.ctypes.data if form == "offsets" else None, n, frames, 12,
                                out.ctypes.data + GB, -1)
        cells[f"host_decode|{form}|0"] = host_verdict(rc, [host_read(out, S.px.nbytes) + (S.px,)])
    out = host_buf(S.px.nbytes)
    rc = L.trpx_decode_host_grouped(signed, code, buf.ctypes.data, buf.size, offs.ctypes.data, None, n, frames, 12, out.ctypes.data + GB, -1)
    cells["host_grouped|offsets|0"] = host_verdict(rc, [host_read(out, S.px.nbytes) + (S.px,)])
    # trpx_stack_open / trpx_stack_read, frame by frame
    h = C.c_void_p()
    rc = L.trpx_stack_open(C.byref(h), signed, buf.ctypes.data, buf.size, offs.ctypes.data, None, n, frames, 12, 0, -1)
    if rc:
        cells["stack_read|offsets|0"] = REFUSED if rc == CORRUPT else f"WRONG: trpx_stack_open returns {rc}"
    else:
        try:
            vs = set()
            for f in range(frames):
                out = host_buf(S.px[f].nbytes)
                rc = L.trpx_stack_read(h, f, code, out.ctypes.data + GB)
                vs.add(host_verdict(rc, [host_read(out, S.px[f].nbytes) + (S.px[f],)]))
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
        out = host_buf(want.nbytes)
        rc = L.trpx_decode_sum_host(code, code_of(np.int64), buf.ctypes.data, buf.size, offs.ctypes.data, n, frames, 12, group, out.ctypes.data + GB, -1)
        cells[f"sum_host|offsets|0:{name}"] = host_verdict(rc, [host_read(out, want.nbytes) + (want,)])
    for which in ("whole", "last"):
        b, h_, w_, want = D.boxes(which)
        out = host_buf(want.nbytes)
        rc = L.trpx_decode_roi_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, n, frames, 12, n, b.ctypes.data, b.shape[0], h_, w_,
                                    out.ctypes.data + GB, -1)
        cells[f"roi_host|offsets|0:{which}"] = host_verdict(rc, [host_read(out, want.nbytes) + (want,)])
    for thr in (1, 1 << 7):
        rows, pos, val = sparse_truth(S.px, thr)
        total = int(rows[-1])
        r_, p_, v_ = host_buf(rows.nbytes), host_buf(pos.nbytes), host_buf(val.nbytes)
        found = C.c_size_t(0)
        rc = L.trpx_decode_sparse_host(code, buf.ctypes.data, buf.size, offs.ctypes.data, n, frames, 12, thr, r_.ctypes.data + GB,
                                       p_.ctypes.data + GB if total else None, v_.ctypes.data + GB if total else None, total, C.byref(found), -1)
        cells[f"sparse_host|offsets|0:{thr}"] = host_verdict(rc, [host_read(r_, rows.nbytes) + (rows,), host_read(p_, pos.nbytes) + (pos,),
                                                                   host_read(v_, val.nbytes) + (val,)])
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
    D = Dev(S)
    cells = {}
    for route in ROUTES:
        with selected("trpx_set_decode_path", route):
            for form in ("offsets", "none"):
                cells[f"decode|{form}|{route}"] = D.decode(form)
    conv = {np.dtype(np.uint16): np.float32, np.dtype(np.int32): np.int64}.get(S.dt)
    if conv:
        for form in ("offsets", "none"):
            cells[f"convert|{form}|0"] = D.decode(form, conv, convert=True)
    for path in (0, 1):
        with selected("trpx_set_locate_path", path):
            cells[f"locate|none|{path}"] = D.locate()
    if D.tuned:
        v, idx, nb = D.build_index()
        cells["build_index|offsets|0"] = v
        if idx is not None:
            for route in (0, 2, 3):
                with selected("trpx_set_decode_path", route):
                    cells[f"indexed|index|{route}"] = D.indexed(idx)
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
    L = lib()
    shape, dt = (3, 7000), np.dtype(np.uint16)
    k1, k0 = nc.make(dt, shape, "K1"), nc.make(dt, shape, "K0")
    assert k1.stream.size != k0.stream.size
    cap = max(k1.stream.size, k0.stream.size)
    terse = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(shape[0] + 1, dtype=torch.int64, device="cuda")
    nbytes = k1.px.nbytes
    out, st = dev_buf(nbytes), status_block()
    ws = torch.empty(L.trpx_decode_workspace_bytes(code_of(dt), shape[1], shape[0], 12) + 256, dtype=torch.uint8, device="cuda")

    def load(S):
        host = np.zeros(cap + 16, np.uint8)
        host[: S.stream.size] = S.stream
        terse.copy_(torch.from_numpy(host))
        offs.copy_(torch.from_numpy(S.offsets.astype(np.int64)))
        out.fill_(FILL)
        st.fill_(77)

    def call():
        return L.trpx_decode(0, code_of(dt), terse.data_ptr(), cap, offs.data_ptr(), shape[1], shape[0], 12, inner_ptr(out), st.data_ptr(),
                             ws.data_ptr(), ws.numel(), stream_ptr())

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
        v = verdict(0, int(st[0].item()), [dev_read(out, nbytes) + (S.px,)])
        want = EXACT if S.kind == "K0" else pinned("decode|offsets|0", S.kind, shape, dt)
        assert v == want, (S.kind, v, want)
