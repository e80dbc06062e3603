"""Generates tests/golden/reference_runs.json: what the REAL reference (oracle/_ref, built by `make -C oracle ref`) makes of
the inputs of the CPU tests that compare against it, so that those tests need no reference build to run:

* differential -- per pixel type, one row per tests/test_oracle.py differential_cases() frame:
  [n, hi, stream bytes, prolix_bits, FNV-1a64 of the reference's stream, FNV-1a64 of the reference's decode of that stream]
* prolix_cli -- the reference `prolix` tool (oracle/_ref/prolix_cli) on the indexed .trpx files of tests/test_cli_tiff.py:
  SHA-256 of the file it was given and of the TIFF it wrote (of the pixels, for many_group_states).

Needs oracle/_ref and the built library (trpx_amd/libtrpx_hip.so, host-only calls): python tests/golden/make_reference_runs.py"""
import hashlib, json, os, re, subprocess, sys, tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import test_cli_tiff as T  # noqa: E402
import test_oracle  # noqa: E402

PROLIX = os.path.join(ROOT, "oracle", "_ref", "prolix_cli")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def ref_prolix(blob, tmp, name):
    """Run the reference `prolix` on a copy of blob; returns the TIFF it wrote."""
    trpx = os.path.join(tmp, name + ".trpx")
    open(trpx, "wb").write(blob)
    subprocess.check_call([PROLIX, trpx], stdout=subprocess.DEVNULL)
    return open(os.path.join(tmp, name + ".tif"), "rb").read()


def main():
    assert O.have_ref() and os.path.exists(PROLIX), "build the reference first: make -C oracle ref"
    differential = {}
    for dt in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.int64):
        rows = []
        for n, hi, px in test_oracle.differential_cases(O, dt):
            s, pb, _ = O.ref_encode(px)
            back = O.ref_decode(s, n, px.dtype, pb)
            rows.append([n, hi, int(s.size), pb, f"{O.fnv1a64(s):016x}", f"{O.fnv1a64(back):016x}"])
        differential[np.dtype(dt).name] = rows
    prolix_cli = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("u8_stack2_16x12", "u16_bigendian_24x24", "i16_single_17x9"):
            blob = T._indexed_trpx(name)
            prolix_cli[name] = dict(trpx_sha256=sha(blob), tif_sha256=sha(ref_prolix(blob, tmp, name)))
        px, blob = T._many_group_states_file()
        ref_prolix(blob, tmp, "many")
        got = T._parse_tiff(os.path.join(tmp, "many.tif")).reshape(px.shape)
        prolix_cli["many_group_states"] = dict(trpx_sha256=sha(blob), pixels_sha256=sha(got.astype("<u2").tobytes()))
    path = os.path.join(ROOT, "tests", "golden", "reference_runs.json")
    text = json.dumps(dict(generator="tests/golden/make_reference_runs.py", reference="senikm/trpx @ 2024_08_07 (oracle/_ref)",
                           differential=differential, prolix_cli=prolix_cli), indent=1)
    text = re.sub(r"\[\s*([^\[\]{}]*?)\s*\]", lambda m: "[" + re.sub(r",\s+", ", ", m.group(1)) + "]", text)   # one row per line
    with open(path, "w") as f:
        f.write(text + "\n")
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
