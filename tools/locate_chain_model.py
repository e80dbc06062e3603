"""CPU model of the chunk links of a position-parallel frame locator ("Locating the frames").

The scheme walks the stack as ONE header chain that ignores frame ends (blocks of 12 values, Terse.hpp:360-372), cut into
chunks of --chunk-bits bits.  Every chunk starts its own chain at its first bit with a guessed previous width of 0, and a
link between neighbours is where the chain coming from chunk c meets the one chunk c + 1 started (same bit position, same
previous width: from there on they are the same chain).  This model measures, on an oracle-encoded stack, how far behind
the chunk boundary the chains meet: the fraction of links that do not close inside the next chunk, and the distances.

    python tools/locate_chain_model.py [--frames 4] [--chunk-bits 16384] [--data synth|poisson3]

CPU only (the oracle encoder and a plain Python walk); a 4-frame 512^2 stack takes about a minute."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from oracle import oracle as O
    from trpx_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--chunk-bits", type=int, default=16384)
    ap.add_argument("--data", default="synth", choices=["synth", "poisson3"])
    a = ap.parse_args()
    n = 512 * 512
    px = O.synth(np.uint16, 0, a.frames, n) if a.data == "synth" else workloads.poisson_u16_np(3.0, 0, a.frames, n)
    stream, _, _ = O.encode_stack(px)
    L = 8 * stream.size
    bits = np.unpackbits(np.concatenate([stream, np.zeros(8, np.uint8)]), bitorder="little")

    def step(pos, w):                                  # one block of the chain: state in front of it -> in front of the next
        x = int(np.packbits(bits[pos:pos + 16], bitorder="little").view("<u2")[0]) if pos + 16 <= bits.size else 0
        if x & 1:
            return pos + 1 + 12 * w, w
        nw, hl = (x >> 1) & 7, 4
        if nw == 7:
            nw += (x >> 4) & 3
            hl = 6
            if nw == 10:
                nw += (x >> 6) & 63
                hl = 12
        return pos + hl + 12 * nw, nw

    C = a.chunk_bits
    n_chunks = (L + C - 1) // C
    dist = []                                          # bits behind the chunk boundary where the chains meet (None: never)
    for c in range(n_chunks - 1):
        pos, w = c * C, 0
        while pos < (c + 1) * C:
            pos, w = step(pos, w)
        yp, yw, d = (c + 1) * C, 0, None
        while max(pos, yp) < L:
            if pos == yp and w == yw:
                d = pos - (c + 1) * C
                break
            if pos <= yp:
                pos, w = step(pos, w)
            else:
                yp, yw = step(yp, yw)
        dist.append(d)
    met = np.array([d for d in dist if d is not None], np.int64)
    print(json.dumps({"data": a.data, "frames": a.frames, "stack_bytes": int(stream.size), "chunk_bits": C, "links": len(dist),
                      "open_past_next_chunk": round(float(np.mean([d is None or d >= C for d in dist])), 4),
                      "never_met": sum(d is None for d in dist),
                      "median_bits": int(np.median(met)) if met.size else None, "max_met_bits": int(met.max()) if met.size else None}))


if __name__ == "__main__":
    main()
