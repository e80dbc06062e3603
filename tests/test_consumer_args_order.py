"""CPU tier: the ten consumers of a decode index (trpx_decode_sum / _roi / _sparse / _dot / _bins / _hist / _corrected / _binned /
_reduce / _sum_labelled and their _host forms) refuse bad arguments with the same code and the same message prefix as the
libraries tests/golden/consumer_arg_codes.json (the first four) and consumer_arg_codes_more.json (the six after them) were
recorded from (tests/golden/make_consumer_arg_codes.py), for every single fault of a fixed list and every pair of two at once:
which fault wins is part of the ABI.  Every call has a fault, so none reaches a device: the device pointers are fake, aligned addresses, the
host pointers small real buffers.  The _host answers were recorded without a device; where one is present only those decided
before the device is looked for (anything but NO_DEVICE) are asked for again."""
import ctypes as C
import itertools
import json
import os

from trpx_amd import _lib

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(_GOLDEN_DIR, "consumer_arg_codes.json")
GOLDEN_MORE = os.path.join(_GOLDEN_DIR, "consumer_arg_codes_more.json")
# which file holds which consumers' answers
RECORDED = {GOLDEN: ("sum", "roi", "sparse", "dot"), GOLDEN_MORE: ("bins", "hist", "corrected", "binned", "reduce", "sum_labelled")}
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
    "bins": dict(labels=IN2, n_bins=37, bins=OUT),
    "hist": dict(group=2, lo=0, shift=0, n_bins=37, hist=OUT),
    "corrected": dict(out_dtype=_lib.F32, dark=IN2, gain=OUT2, out=OUT),
    "binned": dict(out_dtype=_lib.I32, width=512, bin_y=2, bin_x=3, out=OUT),
    "reduce": dict(op=_lib.REDUCE_MAX, group=2, threshold=0, out=OUT),
    "sum_labelled": dict(out_dtype=_lib.I32, labels=IN2, n_out=3, sums=OUT, counts=OUT2),
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
    "bins": [("labels_askew", _set(labels=IN2 + 1)), ("bins_askew", _set(bins=OUT + 4)), ("own", _set(n_bins=4097))],
    "hist": [("hist_askew", _set(hist=OUT + 4)), ("own", _set(n_bins=4097)), ("own2", _set(group=0))],
    "corrected": [("dark_askew", _set(dark=IN2 + 2)), ("gain_askew", _set(gain=OUT2 + 2)), ("out_askew", _set(out=OUT + 2)),
                  ("own", _set(out_dtype=_lib.F64))],
    "binned": [("out_askew", _set(out=OUT + 2)), ("own", _set(bin_x=65)), ("own2", _set(out_dtype=_lib.U8))],
    "reduce": [("out_askew", _set(out=OUT + 1)), ("own", _set(op=7)), ("own2", _set(group=0))],
    "sum_labelled": [("labels_askew", _set(labels=IN2 + 2)), ("sums_askew", _set(sums=OUT + 2)), ("counts_askew", _set(counts=OUT2 + 2)),
                     ("own", _set(n_out=0)), ("own2", _set(n_out=(1 << 20) + 1))],
}
HOST_FAULTS = ["block7", "dtype64", "dtype_unknown", "no_bytes", "frames_gt_bytes", "own", "own2"]


def _need(L, name, a):
    extra = {"sum": ("group",), "dot": ("n_maps",), "bins": ("n_bins",), "hist": ("group", "n_bins"), "reduce": ("group",),
             "sum_labelled": ("n_out",)}.get(name, ())
    first = (a["dtype"], a["op"]) if name == "reduce" else (a["dtype"],)       # (reduce: the op is its second argument)
    return getattr(L, f"trpx_decode_{name}_workspace_bytes")(*first, a["terse_bytes"], a["n_values"], a["n_frames"], a["block"],
                                                             *(a[k] for k in extra))


def _call_ptr(L, name, a):
    front = (a["terse"], a["terse_bytes"], a["offs"], a["index"], a["n_values"], a["n_frames"], a["block"])
    back = (a["status"], a["ws"], max(_need(L, name, a) - a["ws_short"], 0), None)
    if name == "sum":
        return L.trpx_decode_sum(a["dtype"], a["out_dtype"], *front, a["group"], a["sums"], *back)
    if name == "roi":
        return L.trpx_decode_roi(a["dtype"], *front, a["width"], a["boxes"], a["n_boxes"], a["box_h"], a["box_w"], a["out"], *back)
    if name == "sparse":
        return L.trpx_decode_sparse(a["dtype"], *front, a["threshold"], a["row_offsets"], a["positions"], a["values"], a["capacity"], *back)
    if name == "dot":
        return L.trpx_decode_dot(a["dtype"], *front, a["weights"], a["n_maps"], a["dots"], *back)
    if name == "bins":
        return L.trpx_decode_bins(a["dtype"], *front, a["labels"], a["n_bins"], a["bins"], *back)
    if name == "hist":
        return L.trpx_decode_hist(a["dtype"], *front, a["group"], a["lo"], a["shift"], a["n_bins"], a["hist"], *back)
    if name == "corrected":
        return L.trpx_decode_corrected(a["dtype"], a["out_dtype"], *front, a["dark"], a["gain"], a["out"], *back)
    if name == "binned":
        return L.trpx_decode_binned(a["dtype"], a["out_dtype"], *front, a["width"], a["bin_y"], a["bin_x"], a["out"], *back)
    if name == "reduce":
        return L.trpx_decode_reduce(a["dtype"], a["op"], *front, a["group"], a["threshold"], a["out"], *back)
    return L.trpx_decode_sum_labelled(a["dtype"], a["out_dtype"], *front, a["labels"], a["n_out"], a["sums"], a["counts"], *back)


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
    if name == "dot":
        return L.trpx_decode_dot_host(a["dtype"], *front, _BUF["in2"], a["n_maps"], _BUF["out"], -1)
    if name == "bins":
        return L.trpx_decode_bins_host(a["dtype"], *front, _BUF["in2"], a["n_bins"], _BUF["out"], -1)
    if name == "hist":
        return L.trpx_decode_hist_host(a["dtype"], *front, a["group"], a["lo"], a["shift"], a["n_bins"], _BUF["out"], -1)
    if name == "corrected":
        return L.trpx_decode_corrected_host(a["dtype"], a["out_dtype"], *front, _BUF["in2"], _BUF["out2"], _BUF["out"], -1)
    if name == "binned":
        return L.trpx_decode_binned_host(a["dtype"], a["out_dtype"], *front, a["width"], a["bin_y"], a["bin_x"], _BUF["out"], -1)
    if name == "reduce":
        return L.trpx_decode_reduce_host(a["dtype"], a["op"], *front, a["group"], a["threshold"], _BUF["out"], -1)
    return L.trpx_decode_sum_labelled_host(a["dtype"], a["out_dtype"], *front, _BUF["in2"], a["n_out"], _BUF["out"], _BUF["out2"], -1)


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
                    if name == "binned":
                        a.update(width=H_WIDTH)
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


def _of(got, names):
    """the answers of the consumers `names` alone"""
    return {half: {k: v for k, v in got[half].items() if k.split("|")[0].removesuffix("_host") in names} for half in got}


def test_codes_and_prefixes_are_the_recorded_ones():
    L = _lib.lib()
    want = {path: json.load(open(path)) for path in RECORDED}
    assert len(want[GOLDEN]["ptr"]) > 400 and len(want[GOLDEN]["host"]) > 40
    for name in RECORDED[GOLDEN_MORE]:
        mine = _of(want[GOLDEN_MORE], (name,))
        assert len(mine["ptr"]) >= 120 and len(mine["host"]) >= 20, name
    keys = {"ptr": set(), "host": set()}
    for key, _, host, _ in cases():
        keys["host" if host else "ptr"].add(key)
    for path, names in RECORDED.items():                    # both files: exactly the keys the tables generate, no OK
        assert all(v[0] != _lib.OK for half in want[path].values() for v in half.values())
        for half in ("ptr", "host"):
            assert want[path][half].keys() == _of({half: dict.fromkeys(keys[half])}, names)[half].keys(), (path, half)
    want = {half: {**want[GOLDEN][half], **want[GOLDEN_MORE][half]} for half in ("ptr", "host")}
    if L.trpx_device_count():                               # a device: only the _host answers that do not depend on one
        want["host"] = {k: v for k, v in want["host"].items() if v[0] != _lib.ERR_NO_DEVICE}
    got = answers(L, lambda key, host: not host or key in want["host"])
    for half in ("ptr", "host"):
        assert got[half].keys() == want[half].keys()
        wrong = {k: (got[half][k], want[half][k]) for k in want[half] if got[half][k] != want[half][k]}
        assert not wrong, wrong
