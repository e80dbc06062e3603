"""Generates tests/golden/noncanonical.json: the REAL reference's verdict (oracle/_ref, built by `make -C oracle ref`) on valid
streams that no encoder here writes -- restated and padded widths, tests/noncanonical.py -- so that the tests which rely on
"the reference decodes these" need no reference build to run.  Per fixture: the generator's parameters, the FNV-1a64 of the
stream bytes and of the pixels, and whether the reference's decoder gave those pixels back for every frame.  Hashes only.

Needs oracle/_ref: python tests/golden/make_noncanonical.py"""
import json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import noncanonical as nc  # noqa: E402

SHAPE = (4, 1073)


def fixtures():
    """(dtype name, shape, kind, variant, block): every integer type at the tuned block size, two types at another"""
    for dt in nc.ALL_DTYPES:
        for block in ((12, 7) if np.dtype(dt) in (np.dtype(np.uint16), np.dtype(np.int32)) else (12,)):
            for kind in nc.KINDS:
                yield np.dtype(dt).name, SHAPE, kind, 0, block


def entry(dtname, shape, kind, variant, block, with_ref):
    s = nc.make(np.dtype(dtname), shape, kind, variant, block)
    e = dict(dtype=dtname, shape=list(shape), kind=kind, variant=variant, block=block,
             stream=f"{O.fnv1a64(s.stream):016x}", pixels=f"{O.fnv1a64(s.px):016x}")
    if with_ref:
        ok = True
        for f in range(shape[0]):
            try:
                back = O.ref_decode(s.stream[s.offsets[f]: s.offsets[f + 1]], shape[1], s.dt, s.prolix_bits, block)
                ok = ok and back.tobytes() == s.px[f].tobytes()
            except RuntimeError:
                ok = False
        e["ref_decodes"] = bool(ok)
    return e


def text_of(entries):
    return "{\n \"generator\": \"tests/golden/make_noncanonical.py\",\n \"reference\": \"senikm/trpx @ 2024_08_07 (oracle/_ref)\",\n \"fixtures\": [\n" + \
        ",\n".join("  " + json.dumps(e) for e in entries) + "\n ]\n}\n"


def main():
    assert O.have_ref(), "build the reference first: make -C oracle ref"
    path = os.path.join(ROOT, "tests", "golden", "noncanonical.json")
    with open(path, "w") as f:
        f.write(text_of([entry(*fx, True) for fx in fixtures()]))
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
