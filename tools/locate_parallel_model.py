"""CPU model of the position-parallel frame locator (decode_locate.hip), block by block in Python.

Same scheme as the device: chunk chains from guessed states (first bit, previous width 0) with a checkpoint in every window
(the chain's first block start there: bit, previous width or "explicit header", blocks from the chunk's start); links from
each chain to the first checkpoint of a later chunk's chain it lands on, with checkpoints along that walk too; a chase that walks each frame from (its first bit,
0) until it lands on a checkpoint and then finds its last block by block counts along the links; a verification of every
frame by the serial walk; the serial walk from the first failed frame on.  `locate()` returns the offsets and status and the
model's statistics; `main()` runs it on oracle-encoded stacks and prints:

* repair_free: the fraction of frames whose proposed offset verified (no serial repair),
* link_closure: the fraction of chunk chains that met a later chunk's chain within the link cap, and the fraction that met
  the very next chunk's,
* hops_per_frame: links followed per frame by the chase, and its landing walk in blocks.

    python tools/locate_parallel_model.py [--frames 8] [--side 512] [--data synth|poisson3] [--win-bits 4096] [--win-per-chunk 64]

CPU only; a 8-frame 512^2 stack takes about a minute."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXPLICIT = 0xFF


class Stream:
    def __init__(self, data):
        self.data = bytes(data) + bytes(16)
        self.n = len(data)

    def peek(self, bit):                                   # 32 bits from absolute bit `bit` (zeros past the end)
        i = bit >> 3
        if i >= self.n:
            return 0
        return (int.from_bytes(self.data[i:i + 5], "little") >> (bit & 7)) & 0xFFFFFFFF


def header(x):
    """explicit header at x (bit 0 clear) -> (width, header bits)"""
    w, hl = (x >> 1) & 7, 4
    if w == 7:
        w += (x >> 4) & 3
        hl = 6
        if w == 10:
            w += (x >> 6) & 63
            hl = 12
    return w, hl


def chain_step(s, pos, w, max_w):
    """one block of the frame-oblivious chain (12 values; a width above max_w reads as 0) -> (next pos, width, explicit)"""
    x = s.peek(pos)
    if x & 1:
        return pos + 1 + 12 * w, w, False
    nw, hl = header(x)
    if nw > max_w:
        nw = 0
    return pos + hl + 12 * nw, nw, True


def serial_frame(s, fo, n_blocks, nb_last, max_w):
    """walk_frame<false>: the frame's bit count, or None (a width above max_w, or past the stream's end)"""
    limit = 8 * (s.n - fo)
    pos, w = 0, 0
    for b in range(n_blocks):
        if pos >= limit:
            return None
        x = s.peek(8 * fo + pos)
        nv = nb_last if b == n_blocks - 1 else 12
        if x & 1:
            pos += 1 + nv * w
        else:
            w, hl = header(x)
            if w > max_w:
                return None
            pos += hl + nv * w
    if pos > limit or pos // 8 + 1 > limit // 8:
        return None
    return pos


def serial_locate(stream, n_values, n_frames, max_w):
    s = Stream(stream)
    nb = (n_values + 11) // 12
    nb_last = n_values - 12 * (nb - 1)
    offs, fo, ok = [0], 0, True
    for _ in range(n_frames):
        bits = serial_frame(s, fo, nb, nb_last, max_w) if ok and fo < s.n else None
        if bits is None:
            ok = False
        else:
            fo += 1 + bits // 8
        offs.append(fo)
    return np.array(offs, np.int64), 0 if ok else 5


def locate(stream, n_values, n_frames, max_w, win_bits=4096, win_per_chunk=64, link_chunks=4, link_blocks=8192):
    s = Stream(stream)
    nb = (n_values + 11) // 12
    nb_last = n_values - 12 * (nb - 1)
    n_win = (8 * s.n + win_bits - 1) // win_bits
    n_chunks = (n_win + win_per_chunk - 1) // win_per_chunk
    cp = {}                                                # window -> (bit, tag, blocks from its chunk's start)
    ends, links = [], []
    for c in range(n_chunks):                              # 1. chunk chains
        w_lo, w_hi = c * win_per_chunk, min((c + 1) * win_per_chunk, n_win)
        pos, w, blk, last = w_lo * win_bits, 0, 0, -1
        while pos < w_hi * win_bits:
            x = s.peek(pos)
            if pos // win_bits != last:
                last = pos // win_bits
                cp[last] = (pos, w if x & 1 else EXPLICIT, blk)
            pos, w, _ = chain_step(s, pos, w, max_w)
            blk += 1
        ends.append((pos, w, blk))

    def match(pos, w):
        v = cp.get(pos // win_bits)
        return v if v is not None and v[0] == pos and v[1] in (EXPLICIT, w) else None

    met_next, link_bits, ext = 0, [], []
    for c in range(n_chunks):                              # 2. links
        w_hi = min((c + 1) * win_per_chunk, n_win)
        pos, w, blk = ends[c]
        link, e, last = None, {}, -1                       # e: checkpoints of the walk past the chunk (its first 64 windows)
        walked = 0
        while w_hi < n_win and pos < w_hi * win_bits + link_chunks * win_per_chunk * win_bits and walked < link_blocks:
            v = match(pos, w)
            if v is not None:
                link = (pos // win_bits, blk, v[2])
                met_next += pos // win_bits < w_hi + win_per_chunk
                link_bits.append(pos - w_hi * win_bits)
                break
            if pos // win_bits != last:
                last = pos // win_bits
                if last < w_hi + 64:
                    e[last] = (pos, w if s.peek(pos) & 1 else EXPLICIT, blk)
            pos, w, _ = chain_step(s, pos, w, max_w)
            blk += 1
            walked += 1
        links.append(link)
        ext.append(e)

    offs, hops, land, adv = [0], [], [], []                # 3. chase
    st = 0
    for _ in range(n_frames):
        if st < s.n:
            pos, w, rem, a = 8 * st, 0, nb - 1, 0
            v = None
            while a < rem:
                v = match(pos, w)
                if v is not None:
                    break
                pos, w, _ = chain_step(s, pos, w, max_w)
                a += 1
            land.append(a)
            rem -= a
            h = 0
            if v is not None:
                c, blk = pos // win_bits // win_per_chunk, v[2]
                while links[c] is not None and blk + rem >= links[c][1]:
                    g, at, tblk = links[c]
                    rem -= at - blk
                    blk, c = tblk, g // win_per_chunk
                    h += 1
                target = blk + rem
                if target >= ends[c][2]:
                    past = [v for v in ext[c].values() if v[2] <= target]
                    best = max(past, key=lambda e: e[2]) if past else None
                    pos, w, fb = ends[c] if best is None else (best[0], 0 if best[1] == EXPLICIT else best[1], best[2])
                else:
                    best = max((cp[g] for g in range(c * win_per_chunk, min((c + 1) * win_per_chunk, n_win))
                                if g in cp and cp[g][2] <= target), key=lambda e: e[2])
                    pos, w, fb = best[0], 0 if best[1] == EXPLICIT else best[1], best[2]
                adv.append(target - fb)
                for _ in range(target - fb):
                    pos, w, _ = chain_step(s, pos, w, max_w)
            hops.append(h)
            x = s.peek(pos)
            if x & 1:
                fin = pos + 1 + nb_last * w
            else:
                nw, hl = header(x)
                fin = pos + hl + nb_last * nw
            st += 1 + (fin - 8 * st) // 8
        offs.append(st)
    offs = np.array(offs, np.int64)

    flags = []                                             # 4. verification
    for f in range(n_frames):
        fo = int(offs[f])
        bits = serial_frame(s, fo, nb, nb_last, max_w) if fo < s.n else None
        flags.append(bits is not None and fo + 1 + bits // 8 == offs[f + 1])
    bad = [f for f in range(n_frames) if not flags[f]]
    status, repaired = 0, 0
    if bad:                                                # 5. serial repair from the first failed frame
        j = bad[0]
        fo = prop = int(offs[j])
        ok = True
        for f in range(j, n_frames):
            prop_next = int(offs[f + 1])
            if ok and fo == prop and flags[f]:
                nxt = prop_next
            else:
                repaired += 1
                bits = serial_frame(s, fo, nb, nb_last, max_w) if ok and fo < s.n else None
                if bits is None:
                    ok = False
                nxt = fo + 1 + bits // 8 if ok else fo
            offs[f + 1] = nxt
            prop, fo = prop_next, nxt
        status = 0 if ok else 5
    stats = {"frames": n_frames, "chunks": n_chunks, "repair_free": round(1 - len(bad) / max(n_frames, 1), 4),
             "walked_in_repair": repaired,
             "link_closure": round(sum(l is not None for l in links[:-1]) / max(n_chunks - 1, 1), 4),
             "link_next_chunk": round(met_next / max(n_chunks - 1, 1), 4),
             "hops_per_frame": round(float(np.mean(hops)), 2) if hops else 0.0,
             "landing_blocks_median": int(np.median(land)) if land else 0, "landing_blocks_max": int(max(land)) if land else 0,
             "advance_blocks_median": int(np.median(adv)) if adv else 0, "advance_blocks_max": int(max(adv)) if adv else 0,
             "link_bits_median": int(np.median(link_bits)) if link_bits else 0,
             "link_bits_max": int(max(link_bits)) if link_bits else 0}
    return offs, status, stats


def main():
    from oracle import oracle as O
    from trpx_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--data", default="synth", choices=["synth", "poisson3"])
    ap.add_argument("--win-bits", type=int, default=4096)
    ap.add_argument("--win-per-chunk", type=int, default=64)
    a = ap.parse_args()
    n = a.side * a.side
    px = O.synth(np.uint16, 0, a.frames, n) if a.data == "synth" else workloads.poisson_u16_np(3.0, 0, a.frames, n)
    stream, sizes, _ = O.encode_stack(px)
    offsets = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    offs, st, stats = locate(stream, n, a.frames, 16, a.win_bits, a.win_per_chunk)
    assert st == 0 and np.array_equal(offs, offsets), "model offsets differ from the encoder's"
    print(json.dumps({"data": a.data, "side": a.side, "stack_bytes": int(stream.size), "win_bits": a.win_bits,
                      "chunk_bits": a.win_bits * a.win_per_chunk, **stats}))


if __name__ == "__main__":
    main()
