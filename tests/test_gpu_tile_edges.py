"""GPU tests: stream edges of the tiled decoders -- k_unpack_tiles and k_sum_tiles, which are assembled from the tile front end of
unpack_tile.hpp, and k_decode_roi, which keeps a front end of its own and shares only the helpers of codec_common.hpp: a
stream whose device base is 4-byte but not 16-byte aligned (the dword-by-dword window loads; at 4, 8 and 12 mod 16), and a stream
whose buffer ends exactly at its last byte (the last 16-byte load of the last tile is the guarded one).  3 frames of
12 * 1024 + 5 values: one full tile of k_unpack_tiles, two of the summing kernel, and a partial last block.  The truth is the original pixels and their
numpy int64 sums: the codec is lossless, so no decoder is trusted.

What each case can tell: "base4", "base8" and "base12" are the ones that discriminate -- a decoder that took the 16-byte loads
there would read misaligned and return wrong pixels, and the bytes behind align4(total) are 0xFF (tests/alignment.py:
carve_stream), so a load that crosses the stream's end and is used returns wrong pixels too.  "exact_end" runs the guarded
last load on a buffer of exactly the stream's bytes and checks its values; it cannot tell a guarded load from an unguarded one, because the allocator rounds the block up and the bytes behind
the stream are mapped (the same holds for every test that passes enc.stack())."""
import numpy as np
import pytest

from alignment import carve_stream
from gpu_support import encode, mixed, selected, to_np
from gpu_support import sum_truth as truth

pytestmark = pytest.mark.gpu

FRAMES, WIDTH, HEIGHT = 3, 647, 19                       # 647 * 19 = 12 * 1024 + 5
VALUES = WIDTH * HEIGHT
ROUTE_TILED = 2                                          # trpx_set_decode_path: position-parallel walk + k_unpack_tiles
assert VALUES == 12 * 1024 + 5


@pytest.fixture(scope="module", params=[np.uint8, np.int16, np.int32], ids=lambda d: np.dtype(d).name)
def stack(request):
    """(pixels, encoded stack, {case: the stream as that case's device tensor}), made once per pixel type."""
    import torch
    px = mixed(request.param, (FRAMES, VALUES), seed=41)
    enc = encode(px)
    s = enc.stack()
    total = s.numel()
    assert total == enc.total_bytes()
    streams = {}
    for off in (4, 8, 12):                               # that far into a larger buffer, 0xFF behind align4(total)
        streams[f"base{off}"], _, _ = carve_stream(s, off)
        assert streams[f"base{off}"].data_ptr() % 16 == off and streams[f"base{off}"].numel() == total
    streams["exact_end"] = s.clone()                     # a buffer of its own that ends with the stream
    assert streams["exact_end"].numel() == total
    return px, enc, streams


CASES = ["base4", "base8", "base12", "exact_end"]


@pytest.mark.parametrize("case", CASES)
def test_decode_indexed_tiled(stack, case):
    from trpx_amd import codec
    import torch
    px, enc, streams = stack
    with selected("trpx_set_decode_path", ROUTE_TILED):
        back, st = codec.decode(streams[case], enc.frame_offsets, VALUES, FRAMES, px.dtype, index=enc.index)
        torch.cuda.synchronize()
    assert int(st[0].item()) == 0
    assert np.array_equal(to_np(back), px)


@pytest.mark.parametrize("group", [1, FRAMES])
@pytest.mark.parametrize("case", CASES)
def test_decode_sum(stack, case, group):
    from trpx_amd import codec
    import torch
    px, enc, streams = stack
    sums, st = codec.decode_sum(streams[case], enc.frame_offsets, VALUES, FRAMES, px.dtype, group, out_dtype=torch.int64,
                                index=enc.index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0
    assert np.array_equal(to_np(sums), truth(px, group, np.int64))


@pytest.mark.parametrize("case", CASES)
def test_decode_roi_last_rows(stack, case):
    from trpx_amd import codec
    import torch
    px, enc, streams = stack
    box_h = 3                                            # the last rows of the last frame, the frame's last pixel included
    boxes = torch.tensor([[FRAMES - 1, HEIGHT - box_h, 0]], dtype=torch.int32, device="cuda")
    out, st = codec.decode_roi(streams[case], enc.frame_offsets, VALUES, FRAMES, px.dtype, WIDTH, boxes, (box_h, WIDTH),
                               index=enc.index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0
    assert np.array_equal(to_np(out)[0], px[FRAMES - 1].reshape(HEIGHT, WIDTH)[HEIGHT - box_h:])
