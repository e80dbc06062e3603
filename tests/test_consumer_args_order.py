"""CPU tier: the four consumers of a decode index (trpx_decode_sum / _roi / _sparse / _dot and their _host forms) refuse bad
arguments with the same code and the same message prefix as the library tests/golden/consumer_arg_codes.json was recorded from
(tests/golden/make_consumer_arg_codes.py), for every single fault of a fixed list and every pair of two at once: which fault
wins is part of the ABI.  Every call has a fault, so none reaches a device: the device pointers are fake, aligned addresses, the
host pointers small real buffers.  The _host answers were recorded without a device; where one is present only those decided
before the device is looked for (anything but NO_DEVICE) are asked for again."""
import ctypes as C
import itertools
import json
import os

from trpx_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumer_arg_codes.json")
N_VALUES, N_FRAMES, TERSE_BYTES = 512 * 512, 8, 1 << 20
TERSE, OFFS, INDEX, STATUS, WS, OUT, IN2, OUT2, OUT3 = (0x10000 * i for i in range(1, 10))
H_VALUES, H_WIDTH, H_FRAMES, H_BYTES = 48, 8, 2, 64         # the host forms' stack: 2 frames of 6 x 8 in 64 bytes

# what every device-pointer call starts from: the index-free form (no offsets, no index), the workspace exactly as large as
# the entry point's own query says
COMMON = dict(dtype=_lib.U16, terse=TERSE, terse_bytes=TERSE_BYTES, offs=None, index=None, n_values=N_VALUES, n_frames=N_FRAMES,
              block=12, status=STATUS, ws=WS, ws_short=0)
OWN = {
    "sum": dict(out_dtype=_lib.I32, group=2, sums=OUT),
    "roi": dict(width=512, boxes=IN2, n_boxes=3, box_h=4, box_w=5, out=OUT),
    "sparse": dict(threshold=100, row_offsets=OUT, positions=OUT2, values=OUT3, capacity=1000),
    "dot": dict(weights=IN2, n_maps=3, dots=OUT),
}


def _set(**kw):
    return lambda a: a.update(kw)


def _index_alone(a):
    a.update(index=a["index"] or INDEX, offs=None)


def _index_askew(a):
    a.update(index=INDEX + 8, offs=a["offs"] or OFFS)


# the faults, applied in this order (a later one sees what an earlier one left)
FAULTS = [
    ("block7", _set(block=7)),
    ("dtype64", _set(dtype=_lib.U64)),
    ("dtype_unknown", _set(dtype=42)),
    ("no_bytes", _set(terse_bytes=0)),
    ("frames_gt_bytes", lambda a: a.update(n_frames=a["terse_bytes"] + 1)),
    ("ws_null", _set(ws=None)),
    ("ws_short", _set(ws_short=1)),
    ("terse_askew", _set(terse=TERSE + 2)),
    ("offs_askew", _set(offs=OFFS + 4)),
    ("index_askew", _index_askew),
    ("status_askew", _set(status=STATUS + 4)),
    ("ws_askew", _set(ws=WS + 4)),
    ("index_alone", _index_alone),
]
OWN_FAULTS = {
    "sum": [("sums_askew", _set(sums=OUT + 2)), ("own", _set(group=0))],
    "roi": [("boxes_askew", _set(boxes=IN2 + 2)), ("out_askew", _set(out=OUT + 1)), ("own", lambda a: a.update(box_w=a["width"] + 1))],
    "sparse": [("rows_askew", _set(row_offsets=OUT + 4)), ("positions_askew", _set(positions=OUT2 + 2)),
               ("values_askew", _set(values=OUT3 + 1)), ("own", _set(values=None))],
    "dot": [("weights_askew", _set(weights=IN2 + 2)), ("dots_askew", _set(dots=OUT + 4)), ("own", _set(n_maps=17))],
}
HOST_FAULTS = ["block7", "dtype64", "dtype_unknown", "no_bytes", "frames_gt_bytes", "own"]


def _need(L, name, a):
    extra = {"sum": (a.get("group"),), "dot": (a.get("n_maps"),)}.get(name, ())
    return getattr(L, f"trpx_decode_{name}_workspace_bytes")(a["dtype"], a["terse_bytes"], a["n_values"], a["n_frames"], a["block"], *extra)


def _call_ptr(L, name, a):
    front = (a["terse"], a["terse_bytes"], a["offs"], a["index"], a["n_values"], a["n_frames"], a["block"])
    back = (a["status"], a["ws"], max(_need(L, name, a) - a["ws_short"], 0), None)
    if name == "sum":
        return L.trpx_decode_sum(a["dtype"], a["out_dtype"], *front, a["group"], a["sums"], *back)
    if name == "roi":
        return L.trpx_decode_roi(a["dtype"], *front, a["width"], a["boxes"], a["n_boxes"], a["box_h"], a["box_w"], a["out"], *back)
    if name == "sparse":
        return L.trpx_decode_sparse(a["dtype"], *front, a["threshold"], a["row_offsets"], a["positions"], a["values"], a["capacity"], *back)
    return L.trpx_decode_dot(a["dtype"], *front, a["weights"], a["n_maps"], a["dots"], *back)


_BUF = {k: (C.c_uint8 * n)() for k, n in dict(terse=H_BYTES, boxes=64, out=1 << 16, in2=4 * 17 * H_VALUES, out2=1 << 12, out3=1 << 12).items()}


def _call_host(L, name, a):
    front = (_BUF["terse"], a["terse_bytes"], None, a["n_values"], a["n_frames"], a["block"])
    if name == "sum":
        return L.trpx_decode_sum_host(a["dtype"], a["out_dtype"], *front, a["group"], _BUF["out"], -1)
    if name == "roi":
        return L.trpx_decode_roi_host(a["dtype"], *front, a["width"], _BUF["boxes"], a["n_boxes"], a["box_h"], a["box_w"], _BUF["out"], -1)
    if name == "sparse":
        n_found = C.c_size_t(0)
        return L.trpx_decode_sparse_host(a["dtype"], *front, a["threshold"], _BUF["out"], _BUF["out2"], a["values"] and _BUF["out3"],
                                         a["capacity"], C.byref(n_found), -1)
    return L.trpx_decode_dot_host(a["dtype"], *front, _BUF["in2"], a["n_maps"], _BUF["out"], -1)


def cases():
    """(key, entry point's short name, host form?, the arguments) of every call: all single faults, all pairs"""
    for name in OWN:
        faults = FAULTS + OWN_FAULTS[name]
        for host in (False, True):
            todo = [f for f in faults if not host or f[0] in HOST_FAULTS]
            for picked in itertools.chain(itertools.combinations(todo, 1), itertools.combinations(todo, 2)):
                a = dict(COMMON, **OWN[name])
                if host:
                    a.update(terse_bytes=H_BYTES, n_values=H_VALUES, n_frames=H_FRAMES, n_boxes=2, capacity=16)
                    if name == "roi":
                        a.update(width=H_WIDTH, box_h=2, box_w=3)
                for _, apply in picked:
                    apply(a)
                yield f"{name}{'_host' if host else ''}|{'+'.join(f[0] for f in picked)}", name, host, a


def answers(L, wanted=lambda key, host: True):
    """{"ptr": {key: [code, message up to the first colon]}, "host": {...}} of the library L, for the calls that are wanted"""
    got = {"ptr": {}, "host": {}}
    for key, name, host, a in cases():
        if wanted(key, host):
            rc = (_call_host if host else _call_ptr)(L, name, a)
            got["host" if host else "ptr"][key] = [rc, L.trpx_last_error_string().decode().split(":")[0]]
    return got


def test_codes_and_prefixes_are_the_recorded_ones():
    L = _lib.lib()
    want = json.load(open(GOLDEN))
    assert len(want["ptr"]) > 400 and len(want["host"]) > 40
    assert all(v[0] != _lib.OK for half in want.values() for v in half.values())
    if L.trpx_device_count():                               # a device: only the _host answers that do not depend on one
        want["host"] = {k: v for k, v in want["host"].items() if v[0] != _lib.ERR_NO_DEVICE}
    got = answers(L, lambda key, host: not host or key in want["host"])
    for half in ("ptr", "host"):
        assert got[half].keys() == want[half].keys()
        wrong = {k: (got[half][k], want[half][k]) for k in want[half] if got[half][k] != want[half][k]}
        assert not wrong, wrong
