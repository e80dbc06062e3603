"""CPU tests of the non-canonical stream writer (oracle.encode_with) and of the stream kinds of tests/noncanonical.py: valid
streams with restated and padded widths, which the decoder grammar (Terse.hpp:360-372) accepts and no encoder here writes.
The oracle's decoder must give the pixels back; so must the real reference, live where oracle/_ref is built and otherwise by
its recorded verdict (tests/golden/noncanonical.json, written by tests/golden/make_noncanonical.py)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import noncanonical as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda d: np.dtype(d).name   # noqa: E731
SHAPES = [(3, 7000), (4, 1073), (2, 7)]


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_noncanonical", os.path.join(ROOT, "tests", "golden", "make_noncanonical.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("block", [12, 7])
@pytest.mark.parametrize("dt", nc.ALL_DTYPES, ids=IDS)
def test_canonical_arguments_give_the_encoders_bytes(oracle, dt, block):
    for shape in SHAPES:
        px = nc.make(dt, shape, "K1", 0, block).px                   # (the kind only selects the data)
        for f in range(shape[0]):
            want, _ = oracle.encode(px[f], block)
            w = oracle.widths(px[f], block)
            assert oracle.encode_with(px[f], w, None, block).tobytes() == want.tobytes(), (dt, block, shape, f)
            assert oracle.encode_with(px[f], w, np.zeros(w.size, np.uint8), block).tobytes() == want.tobytes()


@pytest.mark.parametrize("dt", nc.ALL_DTYPES, ids=IDS)
def test_widths_out_of_range_are_refused(oracle, dt):
    px = nc.make(dt, (1, 1000), "K0").px[0]
    w = oracle.widths(px)
    assert w.max() > 0
    low = w.copy()
    low[int(np.argmax(w))] -= 1                                      # narrower than the block needs
    with pytest.raises(ValueError):
        oracle.encode_with(px, low)
    high = w.copy()
    high[0] = 8 * np.dtype(dt).itemsize + 1                          # wider than the type
    with pytest.raises(ValueError):
        oracle.encode_with(px, high)
    full = np.full_like(w, 8 * np.dtype(dt).itemsize)                # the type's bit size itself is allowed
    s = oracle.encode_with(px, full)
    assert (oracle.decode(s, px.size, dt) == px).all()
    with pytest.raises(ValueError):
        oracle.encode_with(px, w[:-1])


@pytest.mark.parametrize("block", [12, 7])
@pytest.mark.parametrize("kind", nc.KINDS)
@pytest.mark.parametrize("dt", nc.ALL_DTYPES, ids=IDS)
def test_every_kind_decodes_to_its_pixels(oracle, dt, kind, block):
    for shape in SHAPES:
        for v in range(nc.variants(shape, kind, dt, block)):
            s = nc.make(dt, shape, kind, v, block)
            assert s.offsets[-1] == s.stream.size
            if kind == "K0":
                assert s.stream.tobytes() == oracle.encode_stack(s.px, block)[0].tobytes()
            if kind in ("K1", "K3", "K5") and shape[1] > 100:
                assert s.explicit.any(), "the kind restates no width here"
            if kind in ("K2", "K3") and shape[1] > 100:
                own = np.stack([oracle.widths(s.px[f], block) for f in range(shape[0])])
                assert (s.widths > own).any(), "the kind pads no width here"
            if kind != "K0" and shape[1] > 100:
                assert s.stream.tobytes() != oracle.encode_stack(s.px, block)[0].tobytes()
            for f in range(shape[0]):
                frame = s.stream[s.offsets[f]: s.offsets[f + 1]]
                ctx = (np.dtype(dt).name, kind, block, shape, v, f)
                assert oracle.decode(frame, shape[1], dt, block=block).tobytes() == s.px[f].tobytes(), ctx
                assert oracle.frame_bytes(s.stream[s.offsets[f]:], shape[1], block) == frame.size, ctx      # (located in the stack)
                assert oracle.frame_bytes(frame, shape[1], block) == frame.size, ctx
                if oracle.have_ref():
                    assert oracle.ref_decode(frame, shape[1], dt, s.prolix_bits, block).tobytes() == s.px[f].tobytes(), ("reference",) + ctx


def test_single_placements_reach_every_block_and_width():
    """K4 does what it is for (a check of the fixture): over its variants every placement meets every run width, one restated
    header per frame, and the last-group ones keep the shortened layout inside the true layout's last byte."""
    for shape in [(3, 7000), (130, 388), (2, 3073)]:
        nblk = -(-shape[1] // 12)
        seen, kept = set(), 0
        for v in range(nc.variants(shape, "K4", np.uint16)):
            s = nc.make(np.uint16, shape, "K4", v)
            for f in range(shape[0]):
                (p,) = np.nonzero(s.explicit[f])[0]
                seen.add((int(p), int(s.widths[f, p])))
                kept += s.same_byte[f] is True
        want = {(p, 0 if p == 0 else w) for p in nc.placements(nblk) for w in nc.RUN_WIDTHS}
        assert want <= seen, (shape, sorted(want - seen))
        assert kept >= 3, shape


def test_recorded_reference_verdicts(oracle):
    """tests/golden/noncanonical.json: every fixture regenerates to the recorded hashes, and the real reference decoded it."""
    with open(os.path.join(ROOT, "tests", "golden", "noncanonical.json")) as f:
        rec = json.load(f)
    m = _make_golden()
    want = list(m.fixtures())
    assert len(rec["fixtures"]) == len(want)
    for e, fx in zip(rec["fixtures"], want):
        assert (e["dtype"], tuple(e["shape"]), e["kind"], e["variant"], e["block"]) == fx
        now = m.entry(*fx, with_ref=False)
        assert (now["stream"], now["pixels"]) == (e["stream"], e["pixels"]), fx
        assert e["ref_decodes"] is True, fx
    if oracle.have_ref():                                            # the file is what the generator writes today
        with open(os.path.join(ROOT, "tests", "golden", "noncanonical.json")) as f:
            assert f.read() == m.text_of([m.entry(*fx, True) for fx in want])
