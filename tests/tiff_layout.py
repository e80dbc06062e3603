"""A parser of the grey TIFF layout the tools write, independent of Grey_tif.hpp: for tests/test_cli_tiff.py and the prolix -sum
test of tests/test_gpu_decode_sum.py."""
import struct

import numpy as np


def parse_tiff(path):
    """Independent little/big-endian parser of the reference writer's layout -> [n, h, w] array."""
    b = open(path, "rb").read()
    e = "<" if b[:2] == b"II" else ">"
    ifd = struct.unpack_from(e + "I", b, 4)[0]
    frames = []
    while ifd:
        n = struct.unpack_from(e + "H", b, ifd)[0]
        tags = {}
        for i in range(n):
            tag, typ, cnt = struct.unpack_from(e + "HHI", b, ifd + 2 + 12 * i)
            tags[tag] = struct.unpack_from(e + ("H" if typ == 3 else "I"), b, ifd + 2 + 12 * i + 8)[0]
        kind = {1: "u", 2: "i", 3: "f"}[tags.get(0x153, 1)]
        dt = np.dtype(f"{e}{kind}{tags[0x102] // 8}")
        w, h = tags[0x100], tags[0x101]
        frames.append(np.frombuffer(b, dt, w * h, tags[0x111]).reshape(h, w))
        ifd = struct.unpack_from(e + "I", b, ifd + 2 + 12 * n)[0]
    return np.stack(frames)
