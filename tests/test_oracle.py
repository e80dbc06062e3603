"""CPU tests (no GPU): the oracle restatement is pinned against the reference's golden vectors.

Sources of truth, in order: (1) tests/golden/terse_golden.json -- produced by the REAL reference
(oracle/_ref, generator tests/golden/make_golden.py); (2) the doc-comment known answers of
Terse.hpp:53-57 / :127-154 and SURVEY.md section 8.0; (3) a differential run against what the
reference made of seeded frames (tests/golden/reference_runs.json, generator
tests/golden/make_reference_runs.py), and against oracle/_ref itself when that library is
present in the checkout."""
import json
import os

import numpy as np
import pytest


def _reference_runs():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs.json")))


def _px(case):
    return np.array(case["pixels"], dtype=np.dtype(case["dtype"]))


def test_golden_encode_bit_exact(oracle, golden):
    assert len(golden["cases"]) >= 30
    for c in golden["cases"]:
        px = _px(c)
        s, pb = oracle.encode(px, c["block"])
        assert s.tobytes().hex() == c["stream"], c["name"]
        assert pb == c["prolix_bits"], c["name"]


def test_golden_decode_pixel_exact(oracle, golden):
    for c in golden["cases"]:
        px = _px(c)
        stream = np.frombuffer(bytes.fromhex(c["stream"]), np.uint8)
        back = oracle.decode(stream, px.size, px.dtype, block=c["block"])
        assert (back == px).all(), c["name"]
        assert oracle.frame_bytes(stream, px.size, c["block"]) == stream.size, c["name"]


def test_doc_comment_known_answers(oracle):
    # Terse.hpp:53-57 (block of 3) and SURVEY.md section 8.0 tiny KATs
    assert oracle.encode(np.array([3, 4, 2], np.uint8), 3)[0].tobytes().hex() == "360a"
    assert oracle.encode(np.array([-3, 4, 2], np.int8), 3)[0].tobytes().hex() == "d82400"
    assert oracle.encode(np.zeros(24, np.uint16))[0].tobytes().hex() == "03"
    a = np.array(list(range(12)) + [0] * 12 + [1000] + [0] * 11 + [1023] + [1] * 11 + [65535, 2], np.uint16)
    want = ("0821436587a90b3e803e" + "00" * 13 + "f0ff00020820800002082080000208c037feff050000")
    s, pb = oracle.encode(a)
    assert s.tobytes().hex() == want and pb == 16 and s.size == 45
    # README / Terse.hpp:127-154: iota(-500..499) as int -> 1152 bytes, prolix_bits 10
    s, pb = oracle.encode(np.arange(-500, 500, dtype=np.int32))
    assert s.size == 1152 and pb == 10


def test_stack_is_concatenation(oracle, golden):
    st = golden["stack"]
    px = np.array(st["pixels"], np.uint16)
    data, sizes, pb = oracle.encode_stack(px)
    assert data.tobytes().hex() == st["stream"]
    assert [int(x) for x in sizes] == st["frame_sizes"]
    off = 0
    for f, sz in enumerate(st["frame_sizes"]):   # frame k starts at sum of the sizes before it
        assert (oracle.decode(data[off:off + sz], px.shape[1], np.uint16) == px[f]).all()
        off += sz


def test_synth_anchors_u16(oracle, golden):
    for a in golden["anchors"]:
        if a["dtype"] != "uint16":
            continue
        px = oracle.synth(np.uint16, a["frame"], 1, a["n"])[0]
        assert f"{oracle.fnv1a64(px):016x}" == a["pixels_fnv"]
        s, pb = oracle.encode(px)
        assert s.size == a["size"] and pb == a["prolix_bits"]
        assert f"{oracle.fnv1a64(s):016x}" == a["stream_fnv"]
        assert s[:16].tobytes().hex() == a["first16"]
        assert (oracle.decode(s, px.size, np.uint16) == px).all()


def test_synth_anchor_i32_4096(oracle, golden):
    a = [x for x in golden["anchors"] if x["dtype"] == "int32"][0]
    px = oracle.synth(np.int32, 0, 1, a["n"])[0]
    assert f"{oracle.fnv1a64(px):016x}" == a["pixels_fnv"]
    s, pb = oracle.encode(px)
    assert s.size == a["size"] == 6948595 and pb == a["prolix_bits"] == 25
    assert f"{oracle.fnv1a64(s):016x}" == a["stream_fnv"]


def test_truncated_stream_is_rejected(oracle):
    px = np.arange(100, dtype=np.uint16)
    s, _ = oracle.encode(px)
    with pytest.raises(RuntimeError):
        oracle.decode(s[:-3], px.size, np.uint16)


def test_worst_case_bound_is_tight_enough(oracle):
    # adversarial: every block has a 12-bit header (alternating widths >= 10) and N % 12 != 0 (D7)
    rng = np.random.RandomState(1)
    n = 12 * 50 + 5
    px = np.zeros(n, np.uint16)
    for b in range(51):
        px[12 * b:12 * b + 12] = rng.randint(0, 1 << (15 if b % 2 else 16), size=min(12, n - 12 * b))
        px[12 * b] = (1 << 14) if b % 2 else (1 << 15)
    s, _ = oracle.encode(px)
    assert s.size <= oracle.worst_case_bytes(np.uint16, n)
    assert (oracle.decode(s, n, np.uint16) == px).all()


def differential_cases(oracle, dtype):
    """Seeded (n, hi, pixels) frames inside the reference's validity domain whose oracle stream fits the
    reference's own buffer (D7); tests/golden/make_reference_runs.py records what the reference makes of each."""
    rng = np.random.RandomState(7)
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    top = bits - 2 if dt.kind == "i" else (31 if bits == 32 else bits)
    if bits == 64:
        top = 30   # Terse.hpp:554 calls the C `abs(int)` on 64-bit values: broken above 2^31
    for n in (1, 11, 12, 13, 24, 100, 1000, 4099):
        for hi in (0, 1, 3, min(top, 12), top):
            mag = rng.randint(0, 1 << hi, size=n, dtype=np.int64) if hi else np.zeros(n, np.int64)
            if dt.kind == "i":
                mag = mag * rng.choice([-1, 1], size=n)
            px = mag.astype(dt)
            if oracle.encode(px)[0].size > int(np.ceil(n * (dt.itemsize + 12.0 / (12 * 8)))):
                continue   # defect D7: the reference's own buffer (Terse.hpp:503) overflows here
            yield n, hi, px


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.int64])
def test_live_differential_vs_reference(oracle, dtype):
    """The oracle against the real reference on differential_cases(): against what the reference made of them
    (tests/golden/reference_runs.json: stream size, FNV-1a64 and prolix_bits of its encode, FNV-1a64 of its decode of that
    stream) and, where oracle/_ref is built in this checkout, against the reference itself."""
    dt = np.dtype(dtype)
    want = _reference_runs()["differential"][dt.name]
    cases = list(differential_cases(oracle, dt))
    assert [[n, hi] for n, hi, _ in cases] == [w[:2] for w in want], dtype
    for (n, hi, px), (_, _, size, pb, stream_fnv, back_fnv) in zip(cases, want):
        so, pbo = oracle.encode(px)
        assert so.size == size and f"{oracle.fnv1a64(so):016x}" == stream_fnv and pbo == pb, (dtype, n, hi)
        assert back_fnv == f"{oracle.fnv1a64(px):016x}", (dtype, n, hi)      # the reference expanded this stream to px
        assert (oracle.decode(so, n, dt) == px).all()
        if oracle.have_ref():
            sr, pbr, _ = oracle.ref_encode(px)
            assert so.tobytes() == sr.tobytes() and pbo == pbr, (dtype, n, hi)
            assert (oracle.ref_decode(so, n, dt, pbo) == px).all()
            assert (oracle.decode(sr, n, dt) == px).all()
