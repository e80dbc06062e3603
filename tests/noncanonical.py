"""Valid TERSE streams that no encoder here writes -- the one seeded generator behind tests/test_noncanonical_model.py (CPU),
tests/test_gpu_noncanonical.py (GPU, through tests/noncanonical_dev.py) and tests/golden/make_noncanonical.py.

The project's encoder and the oracle's write CANONICAL streams: a block whose width equals the one before gets the single
"same width" bit, and no width is larger than the block's values need.  The decoder grammar (Terse.hpp:360-372) accepts more:
  restated width   flag 0 + the width code although the width repeats (4, 6 or 12 header bits where a canonical stream has 1);
  padded width     a width larger than the values need.
The stream kinds:
  K0  canonical: oracle.encode's bytes, the control
  K1  restated: every block whose width equals its predecessor's gets an explicit header with probability 0.3
  K2  padded: every block's width grows by 1 .. 3 with probability 0.3, capped at `top`
  K3  both
  K4  single placements: every frame holds exactly ONE restated header, in a frame of one run width (3, 8, 13: restated headers
      of 4, 6, 12 bits), at block 0 (an explicit width 0 at the frame's start), block 1, blocks 255 / 256 / 257, the block before
      the last, the (short) last block, the first block of the frame's last group of 256 blocks.  `variant` shifts which
      (placement, run width) pair frame 0 gets, so that stacks of few frames reach every pair.
  K5  all explicit: every block carries an explicit header; even frames hold width-0 blocks only ("0000" each, no payload), odd
      frames one constant width.
Data stay inside the reference's validity domain, with the `top` of tests/gpu_support.py::fuzz_stack.
Truth is always the pixels returned here, never anything a decoder produced."""
import dataclasses
import zlib

import numpy as np

from oracle import oracle as O

KINDS = ("K0", "K1", "K2", "K3", "K4", "K5")
ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
RUN_WIDTHS = (3, 8, 13)
GROUP_BLOCKS = 256


def top_of(dt) -> int:
    """The widest block the data use: fuzz_stack's for 8 .. 32 bits; 30 for the 64-bit containers, beyond which the reference's
    own 64-bit code is broken (tests/test_oracle.py::differential_cases: Terse.hpp:554 calls the C abs(int))."""
    dt = np.dtype(dt)
    if dt.itemsize == 8:
        return 30
    return 8 * dt.itemsize - (2 if dt.kind == "i" else (1 if dt.itemsize == 4 else 0))


def header_bits(w: int) -> int:
    """Bits of an explicit header of width w, flag included (Terse.hpp:522-533)."""
    return 4 if w < 7 else (6 if w < 10 else 12)


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _values(rng, dt, hi, n, block):
    """[frames, n] pixels whose block b of frame f has exactly width hi[f, b] (unsigned) / hi + 1 (signed), hi > 0: random
    fields below 2^hi, one of them with bit hi - 1 set."""
    dt = np.dtype(dt)
    frames, nblk = hi.shape
    cnt = np.full(nblk, block)
    cnt[-1] = n - (nblk - 1) * block
    h = np.repeat(hi, block, axis=1).astype(np.int64)
    mag = (rng.rand(frames, nblk * block) * (2.0 ** h)).astype(np.int64)
    mag = np.minimum(mag, (np.int64(1) << h) - 1)
    pos = (np.arange(nblk) * block + rng.randint(0, 1 << 30, size=(frames, nblk)) % cnt)          # inside the block's values
    f_idx = np.repeat(np.arange(frames)[:, None], nblk, axis=1)
    lead = np.where(hi > 0, np.int64(1) << np.maximum(hi - 1, 0).astype(np.int64), 0)
    mag[f_idx, pos] |= lead
    mag = mag[:, :n]
    if dt.kind == "i":
        mag = mag * rng.choice([-1, 1], size=mag.shape)
    return mag.astype(dt)


def _mixed_hi(rng, dt, frames, nblk):
    """Runs of one small width (what restating needs), outliers of any width, a stretch of empty blocks."""
    mag_top = top_of(dt) - (1 if np.dtype(dt).kind == "i" else 0)          # (a signed block is one bit wider than its magnitudes)
    base = np.repeat(rng.randint(0, min(mag_top, 6) + 1, size=(frames, (nblk + 39) // 40)), 40, axis=1)[:, :nblk]
    hi = np.where(rng.rand(frames, nblk) < 0.1, rng.randint(0, mag_top + 1, size=(frames, nblk)), base)
    hi[:, nblk // 2: nblk // 2 + nblk // 5] = 0
    return hi


def placements(nblk: int):
    """K4: the blocks that get the one restated header, in the order of the module's docstring; those the frame has, once each."""
    want = [0, 1, 255, 256, 257, nblk - 2, nblk - 1, (nblk - 1) // GROUP_BLOCKS * GROUP_BLOCKS]
    out = []
    for b in want:
        if 0 <= b < nblk and b not in out:
            out.append(b)
    return out


def _frame_bits(w, e, n, block):
    """Bit count of ONE frame written with widths w and explicit flags e (the layout rule, restated here for the fixture)."""
    nblk = w.size
    prev = np.concatenate([[0], w[:-1]])
    hl = np.where((w == prev) & ~e, 1, np.where(w < 7, 4, np.where(w < 10, 6, 12)))
    cnt = np.full(nblk, block)
    cnt[-1] = n - (nblk - 1) * block
    return int((hl + cnt * w).sum())


@dataclasses.dataclass
class Stack:
    dt: np.dtype
    shape: tuple            # (frames, values)
    kind: str
    block: int
    px: np.ndarray          # [frames, values]: the truth
    widths: np.ndarray      # [frames, blocks] u8: as written
    explicit: np.ndarray    # [frames, blocks] bool: headers written in full although the width repeats
    stream: np.ndarray      # u8: the frames' streams, one after the other
    offsets: np.ndarray     # int64 [frames + 1]: the writer's frame offsets
    same_byte: list         # K4: per frame, None or whether the layout WITHOUT the restated header's extra bits ends in the same byte

    @property
    def prolix_bits(self) -> int:
        return int(self.widths.max()) if self.widths.size else 0


def make(dt, shape, kind, variant: int = 0, block: int = 12) -> Stack:
    dt = np.dtype(dt)
    frames, n = shape
    nblk = (n + block - 1) // block
    rng = np.random.RandomState(_seed(dt.name, tuple(shape), kind, variant, block))
    signed = dt.kind == "i"
    same_byte = [None] * frames
    if kind in ("K0", "K1", "K2", "K3"):
        px = _values(rng, dt, _mixed_hi(rng, dt, frames, nblk), n, block)
        w = np.stack([O.widths(px[f], block) for f in range(frames)]).astype(np.int64)
        e = np.zeros((frames, nblk), bool)
        if kind in ("K2", "K3"):
            grow = np.where(rng.rand(frames, nblk) < 0.3, rng.randint(1, 4, size=(frames, nblk)), 0)
            w = np.maximum(w, np.minimum(w + grow, top_of(dt)))
        if kind in ("K1", "K3"):
            prev = np.concatenate([np.zeros((frames, 1), np.int64), w[:, :-1]], axis=1)
            e = (w == prev) & (rng.rand(frames, nblk) < 0.3)
    elif kind == "K4":
        runs = [r for r in RUN_WIDTHS if r <= top_of(dt)]
        P = placements(nblk)
        hi = np.zeros((frames, nblk), np.int64)
        e = np.zeros((frames, nblk), bool)
        for f in range(frames):
            k = f + variant * frames
            p, rw = P[k % len(P)], runs[(k // len(P)) % len(runs)]
            hi[f] = rw - (1 if signed else 0)
            if p == 0:
                hi[f, 0] = 0                                              # block 0 restates the width 0 a frame starts with
            e[f, p] = True
            wf = np.where(hi[f] > 0, hi[f] + (1 if signed else 0), 0)
            last_group = p >= (nblk - 1) // GROUP_BLOCKS * GROUP_BLOCKS and p >= 3     # (blocks 0, 1: the placements of that name)
            if last_group:
                # the true bit count T and the count without the restated header's extra bits end in the same byte where
                # T % 8 >= extra % 8: a few leading blocks of other widths (2, 4, 2, ...: an odd number of bits each) move T there
                extra = header_bits(int(wf[p])) - 1
                done = False
                for lead in range(0, min(24, p - 2)):
                    for pat in ((2, 4), (2,), (4,), (2, 2, 4), (5, 2)):
                        lw = np.array(pat)[np.arange(lead) % len(pat)]
                        trial = wf.copy()
                        trial[2: 2 + lead] = lw
                        if not done and _frame_bits(trial, e[f], n, block) % 8 >= extra % 8:
                            hi[f, 2: 2 + lead] = lw - (1 if signed else 0)
                            wf, done = trial, True
                    if done:
                        break
                same_byte[f] = _frame_bits(wf, e[f], n, block) % 8 >= extra % 8
        px = _values(rng, dt, hi, n, block)
        w = np.stack([O.widths(px[f], block) for f in range(frames)]).astype(np.int64)
        assert (w == np.where(hi > 0, hi + (1 if signed else 0), 0)).all(), "K4: a block's width is not the one asked for"
        prev = np.concatenate([np.zeros((frames, 1), np.int64), w[:, :-1]], axis=1)
        assert (e.sum(axis=1) == 1).all() and (w == prev)[e].all(), "K4: one restated header per frame, on a repeated width"
        if nblk >= 64:
            assert all(s is not False for s in same_byte), "K4: a last-group placement whose shortened layout leaves its byte"
    elif kind == "K5":
        cw = min(5, top_of(dt))
        hi = np.zeros((frames, nblk), np.int64)
        hi[1::2] = cw - (1 if signed else 0)
        px = _values(rng, dt, hi, n, block)
        w = np.stack([O.widths(px[f], block) for f in range(frames)]).astype(np.int64)
        e = np.ones((frames, nblk), bool)
        assert (w[0::2] == 0).all() and (w[1::2] == cw).all()
    else:
        raise ValueError(kind)
    if kind == "K0":
        stream, sizes, _ = O.encode_stack(px, block)
    else:
        stream, sizes = O.encode_stack_with(px, w.astype(np.uint8), e, block)
    offsets = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))]).astype(np.int64)
    return Stack(dt, (frames, n), kind, block, px, w.astype(np.uint8), e, stream, offsets, same_byte)


def variants(shape, kind, dt=np.uint16, block: int = 12) -> int:
    """How many K4 variants of this shape it takes to give every (placement, run width) pair to some frame; 1 elsewhere."""
    if kind != "K4":
        return 1
    frames, n = shape
    pairs = len(placements((n + block - 1) // block)) * len([r for r in RUN_WIDTHS if r <= top_of(dt)])
    return -(-pairs // frames)
