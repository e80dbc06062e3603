"""Views at the weakest alignment include/trpx_hip.h allows, for tests/test_gpu_alignment.py and tests/test_gpu_tile_edges.py.

Every tensor of torch's allocator is at least 256-byte aligned, so a pointer that is aligned to its type only -- a stream at
base + payload_offset of an uploaded file, a view into a larger buffer -- has to be carved out of a larger tensor.  carve() does
that and keeps guards around the view:

  * a buffer a call READS (read_only=True) lies in 0xFF: an element loaded from across the edge is a full-width value, stream
    bits from across the edge are set bits, so a load that crosses the edge and is used changes the result;
  * a buffer a call WRITES lies in -- and is itself prefilled with -- the position-dependent pattern (37 * i + 11) & 0xFF, i the
    byte's position in the room: after the call same_bytes() finds an unwritten byte of the view (it still holds the pattern,
    not the truth) and check() finds a store outside the view, also one of a plausible value such as a constant sentinel's.

No fixtures, no library: tests/test_alignment_model.py runs all of this on CPU tensors and shows that each check can fail."""
import numpy as np

GUARD = 256
SLACK = 128                      # room for every residue mod 128

# residues mod 128 by element size: the thresholds of store_group_lines (unpack_common.hpp) and the 4- / 16-byte tests
RESIDUES = {1: (1, 2, 3, 63, 64, 65, 127), 2: (2, 62, 64, 66, 126), 4: (4, 60, 64, 124), 8: (8,)}
STREAM_RESIDUES = (4, 8, 12, 68)              # mod 16: 4, 8, 12, 4


def align_up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def pattern(nbytes: int, device):
    """uint8 [nbytes]: byte i = (37 * i + 11) & 0xFF.  37 is odd, so 256 successive bytes are all different."""
    import torch
    return (torch.arange(nbytes, dtype=torch.int32, device=device) * 37 + 11).bitwise_and_(255).to(torch.uint8)


def to_bytes(a) -> np.ndarray:
    """The bytes of a torch tensor or numpy array as a flat numpy uint8 array on the host."""
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Check:
    """check() of one carved room: every byte outside the view still holds what was put there."""

    def __init__(self, room, lo: int, hi: int):
        self.room, self.lo, self.hi = room, lo, hi
        self.front = to_bytes(room[:lo]).copy()              # what the guards hold, kept on the host
        self.back = to_bytes(room[hi:]).copy()

    def __call__(self, what="") -> None:
        for name, got, want, base in (("in front of", to_bytes(self.room[:self.lo]), self.front, 0),
                                      ("behind", to_bytes(self.room[self.hi:]), self.back, self.hi)):
            bad = np.flatnonzero(got != want)
            if bad.size:
                i = int(bad[0])
                edge = self.lo - i if base == 0 else i + 1
                raise AssertionError(f"{what}: {bad.size} byte(s) {name} the view changed; the first at distance {edge} from its "
                                     f"edge: {want[i]:#04x} -> {got[i]:#04x}")


def carve(nbytes: int, tdtype, byte_offset: int, device, guard: int = GUARD, read_only: bool = False):
    """(view, room, check): `view` = nbytes bytes as `tdtype` with view.data_ptr() % 128 == byte_offset inside `room`, one uint8
    tensor of guard + 128 + nbytes + guard bytes; check(what) raises AssertionError if a byte of the room outside the view is not
    what carve put there.  read_only: the room is 0xFF (the caller copies its data into the view); otherwise room AND view hold
    pattern()."""
    import torch
    assert 0 <= byte_offset < SLACK and guard >= 128 and guard % 128 == 0      # (the guard keeps the view's residue)
    size = guard + SLACK + nbytes + guard
    if torch.device(device).type == "cpu":                   # (the host allocator promises 64 bytes only: the model tests)
        raw = torch.empty(size + 256, dtype=torch.uint8)
        room = raw[-raw.data_ptr() % 256:][:size]
    else:
        room = torch.empty(size, dtype=torch.uint8, device=device)
    assert room.data_ptr() % 256 == 0, "the allocator's blocks are expected to be 256-byte aligned"
    if read_only:
        room.fill_(0xFF)
    else:
        room.copy_(pattern(room.numel(), device))
    lo = guard + byte_offset
    view = room[lo: lo + nbytes].view(tdtype)
    assert view.data_ptr() % 128 == byte_offset and view.numel() * view.element_size() == nbytes
    assert view.data_ptr() % view.element_size() == 0, "the header asks for pointers aligned to their type"
    return view, room, Check(room, lo, lo + nbytes)


def carve_copy(src, byte_offset: int, device=None, guard: int = GUARD):
    """An input of a call: `src` (a tensor) copied into a read-only carve at `byte_offset`, 0xFF all around it."""
    import torch
    device = src.device if device is None else device
    view, room, check = carve(src.numel() * src.element_size(), src.dtype, byte_offset, device, guard, read_only=True)
    view.view(torch.uint8).copy_(src.contiguous().reshape(-1).view(torch.uint8))
    return view.view(src.shape), room, check


def carve_stream(stream, byte_offset: int, device=None, guard: int = GUARD):
    """A stack as a reader has it inside an uploaded file: `stream` (uint8 [total]) at a base that is `byte_offset` mod 128.
    Bytes [total, align4(total)) are zero, as the encoder leaves them (include/trpx_hip.h, trpx_encode); everything from
    align4(total) on is 0xFF: nothing outside terse[0 .. align4(terse_bytes)) may be read, so set bits there must not matter."""
    assert byte_offset % 4 == 0, "terse is 4-byte aligned"
    device = stream.device if device is None else device
    total = stream.numel()
    view, room, check = carve(total, stream.dtype, byte_offset, device, guard, read_only=True)
    view.copy_(stream)
    pad = align_up(total, 4) - total
    if pad:
        room[check.hi: check.hi + pad] = 0
        check.back[:pad] = 0
    return view, room, check


def same_bytes(got, want, what="") -> None:
    """The defined part of an output equals the truth byte for byte (`got`: tensor or array, `want`: numpy array)."""
    g, w = to_bytes(got), to_bytes(want)
    assert g.size == w.size, (what, g.size, w.size)
    bad = np.flatnonzero(g != w)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} bytes differ from the truth; the first at byte {i}: "
                             f"{g[i]:#04x}, the truth is {w[i]:#04x}")
