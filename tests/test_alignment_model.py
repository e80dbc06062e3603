"""CPU tier: tests/alignment.py can fail.  The carved views of tests/test_gpu_alignment.py on CPU tensors: the residue asked
for is the residue delivered, check() passes on an untouched room and fails for one byte changed next to the view and at the
guard's far end -- also when the byte is overwritten with what a constant-fill sentinel would have held there, which is why the
fill depends on the position --, and the comparison with the truth fails for one byte a call did not write."""
import numpy as np
import pytest
import torch

from alignment import GUARD, RESIDUES, STREAM_RESIDUES, align_up, carve, carve_copy, carve_stream, pattern, same_bytes

CPU = torch.device("cpu")
TYPES = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SENTINEL = 0xA5                                              # what a constant fill would have put everywhere
NBYTES = 3 * 8 * 41                                          # a multiple of every element size, of no line size


@pytest.mark.parametrize("size", sorted(RESIDUES))
def test_the_residue_asked_for_is_delivered(size):
    for read_only in (False, True):
        for off in RESIDUES[size]:
            view, room, check = carve(NBYTES, TYPES[size], off, CPU, read_only=read_only)
            assert view.data_ptr() % 128 == off and view.data_ptr() % size == 0
            assert view.dtype == TYPES[size] and view.numel() * size == NBYTES
            assert room.numel() == GUARD + 128 + NBYTES + GUARD and room.data_ptr() % 256 == 0
            assert view.data_ptr() - room.data_ptr() == GUARD + off
            check()


def test_the_stream_residues_and_the_bytes_behind_a_stream():
    for total in (40, 41, 42, 43):
        stream = torch.arange(1, total + 1, dtype=torch.uint8)
        for off in STREAM_RESIDUES:
            view, room, check = carve_stream(stream, off)
            assert view.data_ptr() % 128 == off and view.data_ptr() % 16 == off % 16 and view.numel() == total
            lo = GUARD + off
            got = room.numpy()
            assert (got[lo: lo + total] == stream.numpy()).all()
            assert (got[lo + total: lo + align_up(total, 4)] == 0).all(), "[total, align4(total)): zero, as the encoder leaves it"
            assert (got[:lo] == 0xFF).all() and (got[lo + align_up(total, 4):] == 0xFF).all()
            check()


def test_the_fills():
    view, room, _ = carve(NBYTES, torch.uint8, 3, CPU)
    want = (37 * np.arange(room.numel()) + 11) & 0xFF
    assert (room.numpy() == want).all() and (view.numpy() == want[GUARD + 3: GUARD + 3 + NBYTES]).all()
    assert len(set(pattern(256, CPU).tolist())) == 256       # no two of 256 neighbours alike
    src = torch.arange(NBYTES // 2, dtype=torch.int16).reshape(3, -1)
    view, room, check = carve_copy(src, 62)
    assert view.shape == src.shape and torch.equal(view, src) and view.data_ptr() % 128 == 62
    outside = np.r_[room.numpy()[:GUARD + 62], room.numpy()[GUARD + 62 + NBYTES:]]
    assert (outside == 0xFF).all()
    check()


def _edges(off):
    """(name, position in the room) of the planted bytes: distance 1 and GUARD - 1 from the view, on either side."""
    lo, hi = GUARD + off, GUARD + off + NBYTES
    return [("front, distance 1", lo - 1), ("front, distance guard - 1", lo - (GUARD - 1)),
            ("back, distance 1", hi), ("back, distance guard - 1", hi + GUARD - 2)]


@pytest.mark.parametrize("read_only", [False, True], ids=["written", "read"])
@pytest.mark.parametrize("value", ["sentinel", "flip", "zero"])
def test_one_byte_outside_the_view_fails_the_check(read_only, value):
    for off in (1, 64, 127):
        for name, pos in _edges(off):
            view, room, check = carve(NBYTES, torch.uint8, off, CPU, read_only=read_only)
            check()
            old = int(room[pos])
            new = {"sentinel": SENTINEL, "flip": old ^ 1, "zero": 0}[value]
            if new == old:                                   # (the pattern passes through every value: not a change here)
                continue
            room[pos] = new
            with pytest.raises(AssertionError, match="the view changed"):
                check(name)
            room[pos] = old
            check()


def test_a_sentinel_byte_is_seen_at_every_position_of_the_guards():
    """With a constant fill a stray store of the fill's own value is invisible.  With the pattern it is visible wherever the
    pattern does not happen to hold that value: at 255 of every 256 positions, and at BOTH of any two neighbours."""
    view, room, check = carve(NBYTES, torch.uint8, 65, CPU)
    lo, hi = GUARD + 65, GUARD + 65 + NBYTES
    seen = 0
    for pos in list(range(lo - GUARD + 1, lo)) + list(range(hi, hi + GUARD - 1)):
        old = int(room[pos])
        room[pos] = SENTINEL
        if old == SENTINEL:
            check()
        else:
            with pytest.raises(AssertionError):
                check()
            seen += 1
        room[pos] = old
    assert seen >= 2 * (GUARD - 1) - 3                       # at most one position in 256 holds the sentinel's value
    check()


def test_one_unwritten_byte_fails_the_comparison_with_the_truth():
    for size in sorted(RESIDUES):
        off = RESIDUES[size][0]
        view, room, check = carve(NBYTES, TYPES[size], off, CPU)
        truth = np.full(NBYTES, 0x5A, np.uint8)
        before = view.view(torch.uint8).numpy().copy()
        skipped = int(np.flatnonzero(before != 0x5A)[7])     # a byte whose prefill is not the truth by chance
        view.view(torch.uint8).copy_(torch.from_numpy(truth))            # "the call": writes every byte ...
        same_bytes(view, truth.view(view.numpy().dtype))
        view.view(torch.uint8)[skipped] = int(before[skipped])           # ... but one
        with pytest.raises(AssertionError, match=f"first at byte {skipped}"):
            same_bytes(view, truth.view(view.numpy().dtype))
        check()                                              # (the guards were never touched)


def test_a_store_one_element_outside_fails_the_check_even_with_a_plausible_value():
    """What a kernel's off-by-one does: the element in front of / behind the view gets a value of the view's own kind."""
    for size in (2, 4, 8):
        view, room, check = carve(NBYTES, TYPES[size], RESIDUES[size][0], CPU)
        view.fill_(7)
        check()
        whole = room[(GUARD + RESIDUES[size][0]) % size:]
        whole = whole[: whole.numel() // size * size].view(TYPES[size])
        first = (view.data_ptr() - whole.data_ptr()) // size
        for pos in (first - 1, first + view.numel()):
            old = whole[pos].clone()
            whole[pos] = 7
            with pytest.raises(AssertionError, match="distance"):
                check()
            whole[pos] = old
            check()
