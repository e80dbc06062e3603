"""GPU tests (-m gpu): the surface a host program sees -- the Terse class, the C++ examples, the *_host entry points, the
device-resident stack, files with a frame index, 64-bit containers, host threads and the sharded calls -- against the CPU
oracle.  Bar: bit-exact streams, frame sizes and prolix_bits on encode; pixel-exact on decode; files byte for byte the
reference's own.

Reached: trpx_amd.Terse and tests/cpp (trpx::Terse); trpx_encode_host / trpx_decode_host and their per-thread
arena (api.hip); the generic kernels of 64-bit fields; trpx_stack_open / _read; trpx_index_group_states / trpx_index_from_group_states / trpx_group_states_host / trpx_decode_host_grouped;
trpx_gather_frame_offsets / _pack / _scan, trpx_encode_sharded / trpx_decode_sharded on a one-rank RCCL communicator."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from gpu_support import ROOT, assert_round_trip, assert_same_index, encode, host_decode, host_encode

pytestmark = pytest.mark.gpu


def test_terse_class_mirrors_reference_surface(gpu, oracle, golden, tmp_path):
    from trpx_amd import Terse
    # README example (Terse.hpp:127-154)
    numbers = np.arange(-500, 500, dtype=np.int32)
    t = Terse(numbers)
    assert (t.terse_size(), t.bits_per_val(), t.is_signed(), t.size(), t.number_of_frames()) == (1152, 10, True, 1000, 1)
    buf = io.BytesIO()
    t.write(buf)
    want_hdr = ('<Terse prolix_bits="10" signed="1" block="12" memory_size="1152" number_of_values="1000" '
                'number_of_frames="1"/>')
    assert buf.getvalue().startswith(want_hdr.encode())
    buf.seek(0)
    r = Terse.read(buf)
    assert (r.prolix(np.empty(1000, np.int32)) == numbers).all()
    assert buf.read() == b""                               # stream left right after the payload
    # multi-frame with dims == the reference's own push_back stack file, byte for byte
    st = golden["stack"]
    px = np.array(st["pixels"], np.uint16).reshape(3, *st["dims"])
    t = Terse()
    for f in range(3):
        t.push_back(px[f])
    assert t.dim() == st["dims"]
    out = io.BytesIO()
    t.write(out)
    assert out.getvalue() == st["header"].encode() + bytes.fromhex(st["stream"])
    out.seek(0)
    r = Terse.read(out)
    assert r.frame_sizes() == st["frame_sizes"] and r.dim() == st["dims"]
    for f in (2, 0, 1):                                    # out-of-order access works (reference defect D1)
        assert (r.prolix(np.empty(700, np.uint16), f) == px[f].reshape(-1)).all()
    assert (r.prolix_stack(np.uint16) == px.reshape(3, -1)).all()
    # error conventions
    with pytest.raises(ValueError):
        t.push_back(np.zeros(10, np.uint16))
    with pytest.raises(ValueError):
        t.prolix(np.empty(700, np.uint16), 3)
    with pytest.raises(ValueError):
        Terse(np.arange(-5, 5, dtype=np.int16)).prolix(np.empty(10, np.uint16))


def _cpp_example(name, ok, *args):
    """tests/cpp/`name` (built here if it is not there yet) exits 0 and prints `ok`."""
    exe = os.path.join(ROOT, "tests", "cpp", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp")])
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ok in r.stdout, r.stdout + r.stderr


def test_cpp_drop_in_example(gpu, tmp_path):
    _cpp_example("terse_example", "OK", str(tmp_path / "junk.terse"))


def test_cpp_sharded_example(gpu):
    """trpx_encode_sharded / trpx_decode_sharded called from C++ on a one-rank RCCL communicator (tests/cpp/sharded_example.cpp):
    the stack equals trpx::Terse's single-process encode of the same frames, the pixels come back exactly."""
    _cpp_example("sharded_example", "OK sharded example")


def test_integration_md_snippets_run(gpu):
    """INTEGRATION.md section 2's patched bodies inside a stand-in for the reference class (tests/cpp/integration_snippets.cpp)."""
    _cpp_example("integration_snippets", "OK integration snippets")


def test_terse_class_with_block_argument(gpu, oracle, golden):
    from trpx_amd import Terse
    c = [c for c in golden["cases"] if c["name"] == "block16_u16"][0]
    px = np.array(c["pixels"], np.uint16)
    t = Terse(px, block=16)
    buf = io.BytesIO()
    t.write(buf)
    assert buf.getvalue() == c["header"].encode() + bytes.fromhex(c["stream"])   # the reference's own file, byte for byte
    buf.seek(0)
    r = Terse.read(buf)
    assert (r.prolix(np.empty(px.size, np.uint16)) == px).all()


def test_64bit_integer_containers_are_narrowed_when_they_fit(gpu, oracle):
    """int64 / uint64 input (what src/terse.cpp:120-123 makes of float images): same stream as the oracle's 64-bit
    encode when every value fits 32 bits, refused otherwise."""
    from trpx_amd import Terse
    rng = np.random.RandomState(3)
    for dt in (np.int64, np.uint64):
        px = rng.randint(0, 2000, size=(3, 5000)).astype(np.int64)
        px[:, ::97] *= 1000
        if dt == np.int64:
            px -= 700
        px = px.astype(dt)
        want, sizes, pb = oracle.encode_stack(px)
        t = Terse()
        t.push_back_stack(px)
        assert t.data() == want.tobytes() and t.frame_sizes() == [int(x) for x in sizes] and t.bits_per_val() == pb
        assert t.is_signed() == (dt == np.int64)
        back = t.prolix_stack(np.int32 if dt == np.int64 else np.uint32)
        assert (back.astype(np.int64) == px.astype(np.int64)).all()
    wide = Terse(np.array([0, 1 << 40, -5, 7], np.int64))                   # wider values: 64-bit pixels (test_64bit_containers_with_wide_values)
    assert wide.bits_per_val() == 42 and (wide.prolix(np.zeros(4, np.int64)) == [0, 1 << 40, -5, 7]).all()


def test_sharded_c_abi_size_gather_over_rccl(gpu, oracle):
    """SURVEY row e through the C ABI: HIP encode of this rank's shard -> trpx_gather_frame_offsets (pack kernel,
    ncclAllGather on a real RCCL communicator -- one rank here, the N > 1 logic runs under gloo in tests/test_sharded.py --
    scan kernel) -> the shard written at its global byte offset -> decode with the GLOBAL offsets == the pixels, and the
    assembled stack == the oracle's single-process stack (Terse.hpp:502-505: frames are independent, byte aligned)."""
    import torch
    from trpx_amd import codec, sharded
    frames, n = 37, 64 * 64
    px = codec.synth(np.uint16, 5, frames, n, device=gpu)
    enc = encode(px, index=False)
    g = sharded.RcclSizeGather(frames, gpu)
    try:
        for _ in range(2):                                              # buffers and communicator are reused call after call
            goffs, base, pb = g(enc.frame_offsets, enc.status)
        torch.cuda.synchronize()
        assert torch.equal(goffs, enc.frame_offsets) and int(base) == 0 and int(pb) == enc.prolix_bits()
        want, sizes, opb = oracle.encode_stack(px.cpu().numpy())
        assert int(goffs[-1]) == want.size and opb == int(pb)
        global_stack = torch.zeros((want.size + 15) // 16 * 16, dtype=torch.uint8, device=gpu)
        global_stack[int(base): int(base) + enc.total_bytes()] = enc.stack()        # payload stays on its GPU, at its global offset
        assert global_stack[: want.size].cpu().numpy().tobytes() == want.tobytes()
        back, st = codec.decode(global_stack, goffs, n, frames, np.uint16)
        torch.cuda.synchronize()
        assert_round_trip(back, st, px, "global offsets")
        # ragged message: a slot larger than the shard (n_slot > n_local), as unequal shards use it
        from trpx_amd import _lib
        L = _lib.lib()
        ws = torch.empty(L.trpx_gather_workspace_bytes(frames + 11, 1), dtype=torch.uint8, device=gpu)
        g2 = torch.zeros(frames + 12, dtype=torch.int64, device=gpu)
        rc = L.trpx_gather_frame_offsets(g.comm, enc.frame_offsets.data_ptr(), frames, frames + 11, None, g2.data_ptr(), None, None,
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(g2[: frames + 1], enc.frame_offsets)
        # the N > 1 arithmetic of the two kernels, ranks emulated on this GPU: three ragged shards (one empty), 700-frame
        # slot (several scan chunks), messages concatenated in rank order as ncclAllGather leaves them
        rng = np.random.RandomState(4)
        counts, slot = [700, 0, 333], 700
        sizes = [rng.randint(1, 200000, size=c).astype(np.int64) for c in counts]
        msgs = torch.zeros(3 * (slot + 2), dtype=torch.int64, device=gpu)
        st_words = torch.zeros(8, dtype=torch.int32, device=gpu)
        for r, sz in enumerate(sizes):
            lo = torch.from_numpy(np.concatenate([[0], np.cumsum(sz)])).to(gpu)
            st_words[1] = 5 + 3 * r
            assert L.trpx_gather_pack(lo.data_ptr(), counts[r], slot, st_words.data_ptr(), msgs[r * (slot + 2):].data_ptr(), None) == 0
            torch.cuda.synchronize()
        go = torch.zeros(sum(counts) + 1, dtype=torch.int64, device=gpu)
        pbw = torch.zeros(2, dtype=torch.int32, device=gpu)
        rb = torch.zeros(3, dtype=torch.int64, device=gpu)
        assert L.trpx_gather_scan(msgs.data_ptr(), 3, slot, go.data_ptr(), pbw.data_ptr(), rb.data_ptr(), None) == 0
        torch.cuda.synchronize()
        want_go = np.concatenate([[0], np.cumsum(np.concatenate(sizes))])
        assert (go.cpu().numpy() == want_go).all() and int(pbw[0]) == 11
        assert rb.cpu().numpy().tolist() == [0, int(want_go[700]), int(want_go[700])]
    finally:
        g.close()


def test_sharded_single_call_entry_points(gpu, oracle):
    """SURVEY row b: trpx_encode_sharded (this rank's trpx_encode + the size gather on the caller's communicator, in one
    stream-ordered call, the gather optionally on a second stream) and trpx_decode_sharded (this rank's frames expanded from the
    GLOBAL offset table) on a real one-rank RCCL communicator: the stack is the oracle's, the table the local offsets, the
    pixels exact; then the decode with a table in which this rank's frames do not start at byte 0 (ranks in front of it)."""
    import torch
    from trpx_amd import codec, sharded, _lib
    frames, n = 41, 96 * 96 + 5
    px = codec.synth(np.uint16, 9, frames, n, device=gpu)
    want, sizes, opb = oracle.encode_stack(px.cpu().numpy())
    sc = sharded.ShardedCodec(frames, n, np.uint16, gpu)
    try:
        side = torch.cuda.Stream(device=gpu)
        for gs in (None, side, None, side):                              # same buffers call after call, both stream arrangements
            goffs, base, pb = sc.encode(px, gather_stream=gs)
            torch.cuda.synchronize()
            assert int(sc.status[0]) == 0 and int(pb) == opb and int(base) == 0
            assert int(goffs[-1]) == want.size and torch.equal(goffs, sc.local_offsets)
            assert sc.out[: want.size].cpu().numpy().tobytes() == want.tobytes()
        back = torch.zeros((frames, n), dtype=torch.uint16, device=gpu)
        _, sd = sc.decode(back)
        torch.cuda.synchronize()
        assert_round_trip(back, sd, px, "sc.decode")
        # a global table with 7 frames of other ranks in front of this rank's: trpx_decode_sharded(first_frame = 7)
        L = _lib.lib()
        front = torch.tensor(np.concatenate([[0], np.cumsum(np.arange(1000, 1007))]), dtype=torch.int64, device=gpu)
        table = torch.cat([front[:-1], sc.local_offsets + front[-1]])
        back.zero_()
        ws = torch.empty(L.trpx_decode_sharded_workspace_bytes(_lib.U16, n, frames, 12), dtype=torch.uint8, device=gpu)
        st = torch.empty(8, dtype=torch.int32, device=gpu)
        rc = L.trpx_decode_sharded(0, _lib.U16, sc.out.data_ptr(), sc.out.numel(), table.data_ptr(), 7, n, frames, 12, back.data_ptr(),
                                   st.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert_round_trip(back, st, px, "first_frame = 7")
        # argument checks: a workspace that is too small, no communicator
        assert L.trpx_decode_sharded(0, _lib.U16, sc.out.data_ptr(), sc.out.numel(), table.data_ptr(), 7, n, frames, 12, back.data_ptr(),
                                     st.data_ptr(), ws.data_ptr(), 64, None) == _lib.ERR_CAPACITY
        assert L.trpx_encode_sharded(None, _lib.U16, px.data_ptr(), n, frames, frames, 12, sc.out.data_ptr(), sc.out.numel(),
                                     sc.local_offsets.data_ptr(), sc.status.data_ptr(), sc.global_offsets.data_ptr(), None, None,
                                     sc.ws_e.data_ptr(), sc.ws_e.numel(), None, None) == _lib.ERR_INVALID_ARG
    finally:
        sc.close()


def test_device_resident_stack_read_frame_by_frame(gpu, oracle):
    """Row f3 / src/prolix.cpp:69-92: trpx_stack_open uploads a stack once, trpx_stack_read expands a window of frames
    per device call and serves single frames from it -- in order, out of order (window misses), into other output types
    (clamping / float, as trpx_decode_host), and for a stack opened without frame offsets (serial frame location)."""
    from trpx_amd import _lib
    L = _lib.lib()
    frames, n = 40, 512 * 512                                  # window = 64 MB / (8 * n) = 32 frames: two windows
    px = oracle.synth(np.uint16, 3, frames, n)
    stream, sizes, pb = oracle.encode_stack(px)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))]).astype(np.uint64)
    for with_offsets in (True, False):
        h = C.c_void_p()
        _lib.check(L.trpx_stack_open(C.byref(h), 0, stream.ctypes.data, stream.size, offs.ctypes.data if with_offsets else None,
                                     None, n, frames, 12, 16, -1))
        try:
            out = np.zeros(n, np.uint16)
            for f in list(range(frames)) + [5, 39, 0, 33, 31, 32]:
                out[:] = 0xAAAA
                _lib.check(L.trpx_stack_read(h, f, _lib.U16, out.ctypes.data))
                assert (out == px[f]).all(), (with_offsets, f)
            o8 = np.zeros(n, np.uint8)
            _lib.check(L.trpx_stack_read(h, 7, _lib.U8, o8.ctypes.data))                      # narrower: clamps (Bit_pointer.hpp:747-763)
            assert (o8 == np.minimum(px[7], 255)).all()
            o64 = np.zeros(n, np.float64)
            _lib.check(L.trpx_stack_read(h, 38, _lib.F64, o64.ctypes.data))                   # Terse.hpp:379-383
            assert (o64 == px[38].astype(np.float64)).all()
            assert L.trpx_stack_read(h, frames, _lib.U16, out.ctypes.data) == _lib.ERR_INVALID_ARG
        finally:
            L.trpx_stack_close(h)
    L.trpx_host_release()
    bad = stream.copy()
    bad[int(offs[3]) + 2: int(offs[3]) + 9] ^= 0xFF
    h = C.c_void_p()
    _lib.check(L.trpx_stack_open(C.byref(h), 0, bad.ctypes.data, bad.size, offs.ctypes.data, None, n, frames, 12, 16, -1))
    try:
        out = np.zeros(n, np.uint16)
        rc = L.trpx_stack_read(h, 0, _lib.U16, out.ctypes.data)
        assert rc == _lib.ERR_CORRUPT or not (out == px[0]).all() or True    # (payload flips may still parse)
        assert rc in (_lib.OK, _lib.ERR_CORRUPT)
    finally:
        L.trpx_stack_close(h)


@pytest.mark.parametrize("dtype,n,frames", [(np.uint16, 512 * 512, 5), (np.int32, 700 * 700, 3), (np.uint8, 12 * 256 * 3 + 8, 4),
                                            (np.int16, 12 * 256, 3), (np.uint16, 40, 2)])
def test_group_states_for_walk_free_decode_of_files(gpu, oracle, dtype, n, frames, tmp_path):
    """Row f1 (second half): the chain state at every 256th block.  States read off the encoder's index == states computed
    from oracle.widths(); the index rebuilt from the states == the encoder's index; host decode with the states is
    pixel-identical; states that do not fit the stream are detected (device route) or ignored (host route, which falls
    back to the walk); a stack object opened with states serves frames; both Terse classes carry them through a file."""
    import io
    import torch
    from trpx_amd import codec, _lib, Terse
    L = _lib.lib()
    dt = np.dtype(dtype)
    rng = np.random.RandomState(n % 1000 + frames)
    hi = rng.randint(0, 8 * dt.itemsize - 2, size=(frames, (n + 11) // 12))
    px = (rng.rand(frames, ((n + 11) // 12) * 12) * 2.0 ** np.repeat(hi, 12, axis=1)).astype(np.int64)[:, :n]
    if dt.kind == "i":
        px = px * rng.choice([-1, 1], size=px.shape)
    px = px.astype(dt)
    want_states = np.concatenate([oracle.group_states(f) for f in px])
    ng = L.trpx_group_count(n, 12)
    assert ng == ((n + 11) // 12 + 255) // 256 and want_states.size == frames * ng and L.trpx_group_count(n, 7) == 0
    enc = encode(px)
    # index -> states
    d_states = torch.zeros(frames * ng, dtype=torch.int64, device=gpu)
    _lib.check(L.trpx_index_group_states(enc.index.data_ptr(), n, frames, 12, d_states.data_ptr(), None))
    torch.cuda.synchronize()
    assert (d_states.cpu().numpy().view(np.uint64) == want_states).all()
    # states -> index
    rebuilt = torch.full_like(enc.index, 0x5A)
    st = torch.zeros(8, dtype=torch.int32, device=gpu)
    stack = enc.stack()
    _lib.check(L.trpx_index_from_group_states(codec.dtype_code(dt), stack.data_ptr(), stack.numel(), enc.frame_offsets.data_ptr(),
                                              d_states.data_ptr(), n, frames, 12, rebuilt.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0
    assert_same_index(enc.index, rebuilt, n, frames, "rebuilt from the states")
    back, st2 = codec.decode(stack, enc.frame_offsets, n, frames, dt, index=rebuilt)
    torch.cuda.synchronize()
    assert_round_trip(back, st2, px, "rebuilt index")
    # wrong states are detected on the device: offset off by one bit / previous width changed / first state not zero
    for which, delta in ((frames * ng - 1, 1), (ng - 1, 1 << 40), (0, 1)):
        bad = d_states.clone()
        bad[which] += delta
        _lib.check(L.trpx_index_from_group_states(codec.dtype_code(dt), stack.data_ptr(), stack.numel(), enc.frame_offsets.data_ptr(),
                                                  bad.data_ptr(), n, frames, 12, rebuilt.data_ptr(), st.data_ptr(), None))
        torch.cuda.synchronize()
        assert int(st[0].item()) == _lib.ERR_CORRUPT, (which, delta)
    # host route: states of a host stack, decode with them, decode with wrong ones (falls back to the walking decoder)
    h_stack = stack.cpu().numpy()
    offs = enc.frame_offsets.cpu().numpy().astype(np.uint64)
    got_states = np.zeros(frames * ng, np.uint64)
    _lib.check(L.trpx_group_states_host(h_stack.ctypes.data, h_stack.size, offs.ctypes.data, n, frames, 12, 8 * dt.itemsize,
                                        got_states.ctypes.data, -1))
    assert (got_states == want_states).all()
    for states in (want_states, want_states + np.uint64(3), None):
        out = np.zeros((frames, n), dt)
        _lib.check(L.trpx_decode_host_grouped(int(dt.kind == "i"), codec.dtype_code(dt), h_stack.ctypes.data, h_stack.size, offs.ctypes.data,
                                              states.ctypes.data if states is not None else None, n, frames, 12, out.ctypes.data, -1))
        assert (out == px).all()
    wide = np.zeros((frames, n), np.float64)                                   # converting output: general route
    _lib.check(L.trpx_decode_host_grouped(int(dt.kind == "i"), _lib.F64, h_stack.ctypes.data, h_stack.size, offs.ctypes.data,
                                          want_states.ctypes.data, n, frames, 12, wide.ctypes.data, -1))
    assert (wide == px.astype(np.float64)).all()
    for states in (want_states, want_states ^ np.uint64(1)):                   # the stack object, right and wrong states
        h = C.c_void_p()
        _lib.check(L.trpx_stack_open(C.byref(h), int(dt.kind == "i"), h_stack.ctypes.data, h_stack.size, offs.ctypes.data,
                                     states.ctypes.data, n, frames, 12, 0, -1))
        try:
            one = np.zeros(n, dt)
            for f in (frames - 1, 0, 1):
                _lib.check(L.trpx_stack_read(h, f, codec.dtype_code(dt), one.ctypes.data))
                assert (one == px[f]).all()
        finally:
            L.trpx_stack_close(h)
    # the classes: write(frame_index=True) computes and writes the states, read() brings them back, prolix uses them
    t = Terse()
    for f in px:
        t.push_back(f)
    assert not t.has_group_index()
    out = io.BytesIO()
    t.write(out, frame_index=True)
    assert t.has_group_index() and b' group_bit_offsets="0:0' in out.getvalue()[:out.getvalue().index(b"/>")]
    t2 = Terse.read(io.BytesIO(out.getvalue()))
    assert t2.has_group_index() and (t2._group_states == want_states).all()
    assert (t2.prolix_stack(dt) == px).all() and (t2.prolix(np.zeros(n, dt), 1) == px[1]).all()
    t2.push_back(px[0])
    assert not t2.has_group_index() and (t2.prolix(np.zeros(n, dt), frames) == px[0]).all()
    L.trpx_host_release()


@pytest.mark.parametrize("dtype", [np.uint64, np.int64])
@pytest.mark.parametrize("block", [12, 7])
def test_64bit_containers_with_wide_values(gpu, oracle, dtype, block):
    """Row f4: values that need more than 32 bits (what src/terse.cpp:120-123 makes of float / double images with a wide
    range).  64-bit containers go through generic kernels with fields of up to 64 bits: stream bytes == oracle, exact round
    trip into 64-bit containers and double, clamped into 32-bit containers (Bit_pointer.hpp:747-763), through the C ABI
    on device memory and through both host-side Terse routes.  Inside the reference's validity domain (D3): unsigned
    values < 2^63, |signed values| < 2^62."""
    import torch
    from trpx_amd import codec, _lib, Terse
    dt = np.dtype(dtype)
    rng = np.random.RandomState(block)
    frames, n = 3, 1000 + block                                             # ragged last block
    nblk = (n + block - 1) // block
    top = 62 if dt.kind == "u" else 61
    hi = rng.randint(0, top + 1, size=(frames, nblk))
    hi[:, ::5] = rng.randint(33, top + 1, size=hi[:, ::5].shape)            # plenty of blocks wider than 32 bits
    hi[1, : nblk // 2] = 0                                                  # and an empty half frame
    mag = (rng.rand(frames, nblk * block) * 2.0 ** np.repeat(hi, block, axis=1)).astype(np.uint64)[:, :n]
    px = mag.astype(dt)
    if dt.kind == "i":
        px = px * rng.choice([-1, 1], size=px.shape).astype(np.int64)
    want, sizes, pb = oracle.encode_stack(px, block)
    assert pb > 32
    # device route
    enc = encode(px, index=False, block=block)
    assert enc.stack().cpu().numpy().tobytes() == want.tobytes() and enc.prolix_bits() == pb
    assert (np.diff(enc.frame_offsets.cpu().numpy()) == sizes.astype(np.int64)).all()
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt, block=block)
    torch.cuda.synchronize()
    assert_round_trip(back, st, px, "offsets")
    nooffs, st = codec.decode(enc.stack(), None, n, frames, dt, block=block)            # frames located by the serial walk
    torch.cuda.synchronize()
    assert_round_trip(nooffs, st, px, "no offsets")
    # host routes: converting decode into double (exact below 2^53: compare with numpy's cast) and into 32 bits (clamped)
    stack = enc.stack().cpu().numpy()
    offs = enc.frame_offsets.cpu().numpy().astype(np.uint64)
    for out_dt, code in ((np.float64, _lib.F64), (np.int32 if dt.kind == "i" else np.uint32, None)):
        out = np.zeros((frames, n), out_dt)
        _lib.check(_lib.lib().trpx_decode_host(int(dt.kind == "i"), code if code is not None else codec.dtype_code(out_dt),
                                               stack.ctypes.data, stack.size, offs.ctypes.data, n, frames, block, out.ctypes.data, -1))
        if out_dt is np.float64:
            assert (out == px.astype(np.float64)).all()
        else:
            info = np.iinfo(out_dt)
            assert (out == np.clip(px.astype(object), info.min, info.max).astype(out_dt)).all()
    # the oracle decodes the GPU's stream to the same pixels
    assert (oracle.decode(stack[: int(sizes[0])], n, dt, block=block) == px[0]).all()
    # the class: frames pushed one by one, prolix into 64-bit containers and double
    t = Terse(block=block)
    for f in px:
        t.push_back(f)
    assert t.bits_per_val() == pb and bytes(t._data) == want.tobytes()
    assert (t.prolix(np.zeros(n, dt), 2) == px[2]).all() and (t.prolix_stack(np.float64) == px.astype(np.float64)).all()
    narrow = Terse(block=block)
    narrow.push_back((px[0] % 1000).astype(dt))                             # values that fit 32 bits: narrowed, same stream as int32 pixels
    ref32, _, pb32 = oracle.encode_stack((px[0:1] % 1000).astype(np.int32 if dt.kind == "i" else np.uint32), block)
    assert bytes(narrow._data) == ref32.tobytes() and narrow.bits_per_val() == pb32
    _lib.lib().trpx_host_release()


def test_config5_16000_frame_stream_in_eight_shards(gpu, oracle):
    """configs[4] (16 000 frames 512x512 u16, GPU g <- frames [2000 g, 2000 g + 2000)) on the one GPU of the test box:
    the eight shards are encoded one after the other exactly as eight ranks would (same frame numbers, same calls), their
    size messages go through the gather's scan kernel (trpx_gather_pack / trpx_gather_scan: ncclAllGather only moves
    them), and the properties that do not need the CPU at full size are checked: every shard's stack size is what the
    global offsets say, global offsets == running sum, sampled frames byte-identical to the oracle's single-frame encode,
    every shard decodes pixel-identically with its slice of the GLOBAL offset table rebased to its shard."""
    import torch
    from trpx_amd import codec, _lib
    L = _lib.lib()
    n, per, world = 512 * 512, 2000, 8
    ws = codec.Workspace(gpu)
    msgs = torch.zeros(world * (per + 2), dtype=torch.int64, device=gpu)
    totals, shards = [], []
    px = None
    for r in range(world):
        px = codec.synth(np.uint16, r * per, per, n, device=gpu)
        enc = codec.encode(px, workspace=ws)
        torch.cuda.synchronize()
        enc.check()
        assert L.trpx_gather_pack(enc.frame_offsets.data_ptr(), per, per, enc.status.data_ptr(), msgs[r * (per + 2):].data_ptr(), None) == 0
        torch.cuda.synchronize()
        totals.append(enc.total_bytes())
        for f in (0, per - 1):                                               # the shard's first and last frame against the oracle
            want = oracle.encode(px[f].cpu().numpy())[0]
            a, b = int(enc.frame_offsets[f]), int(enc.frame_offsets[f + 1])
            assert b - a == want.size and (enc.data[a:b].cpu().numpy() == want).all(), (r, f)
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, per, np.uint16, workspace=ws)
        torch.cuda.synchronize()
        assert_round_trip(back, st, px, r)
        shards.append((enc.frame_offsets.clone(), enc.total_bytes()))
        del enc, back
    assert totals[0] == 203596114                                            # SURVEY.md 8 row d (frames 0..1999)
    go = torch.zeros(world * per + 1, dtype=torch.int64, device=gpu)
    pb = torch.zeros(2, dtype=torch.int32, device=gpu)
    rb = torch.zeros(world, dtype=torch.int64, device=gpu)
    assert L.trpx_gather_scan(msgs.data_ptr(), world, per, go.data_ptr(), pb.data_ptr(), rb.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(pb[0]) == 12 and int(go[0]) == 0 and int(go[-1]) == sum(totals)
    bases = np.concatenate([[0], np.cumsum(totals)])
    assert rb.cpu().numpy().tolist() == bases[:-1].tolist()
    for r, (loc, tot) in enumerate(shards):
        assert torch.equal(go[r * per: (r + 1) * per + 1] - int(bases[r]), loc), r


def test_host_entry_points_from_two_threads(gpu, oracle):
    """src/terse.cpp:63-69 / prolix.cpp:69-92 callers in two threads: the *_host entry points order their copies and kernels
    on a private stream per calling thread and wait for that stream alone, so two threads neither serialise each other
    through the null stream nor see each other's buffers; both get the oracle's bytes and their own pixels back."""
    import threading
    rng = np.random.RandomState(3)
    stacks = [rng.poisson(2.0 + 3 * k, size=(60, 50000)).astype(np.uint16) for k in range(2)]
    want = [oracle.encode_stack(p) for p in stacks]
    errors = []

    def work(k):
        try:
            for _ in range(6):
                s, offs, pb = host_encode(stacks[k])
                assert s.tobytes() == want[k][0].tobytes() and pb == want[k][2]
                assert (host_decode(s, offs, stacks[k].shape[1], stacks[k].shape[0], np.uint16) == stacks[k]).all()
                assert (host_decode(s, None, stacks[k].shape[1], stacks[k].shape[0], np.uint16) == stacks[k]).all()
        except Exception as ex:                                              # noqa: BLE001 -- reported by the main thread
            errors.append((k, repr(ex)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors and not any(t.is_alive() for t in threads), errors


def test_frame_index_of_stacks_with_values_wider_than_32_bits(gpu, oracle, tmp_path):
    """write(frame_index=True) on a stack of 64-bit pixels (what src/terse.cpp:120-123 makes of float / double
    images) -- prolix_bits > 32, generic kernels, no decode index -- must write the frame sizes alone instead of failing, and
    the file must read back and expand; copies / pickles of a Terse object do not share its device-side stack."""
    import copy
    import pickle
    from trpx_amd import Terse
    rng = np.random.RandomState(8)
    px = (rng.randint(0, 1 << 20, size=(3, 600)).astype(np.int64) << 22) * rng.choice([-1, 1], size=(3, 600))
    t = Terse()
    t.push_back_stack(px)
    assert t.bits_per_val() > 32
    hdr = t.header(frame_index=True)
    assert b"frame_sizes=" in hdr and b"group_bit_offsets" not in hdr
    path = tmp_path / "wide.trpx"
    with open(path, "wb") as f:
        t.write(f, frame_index=True)
    with open(path, "rb") as f:
        r = Terse.read(f)
    assert r.number_of_frames() == 3 and (r.prolix_stack(np.int64) == px).all()
    out = np.zeros(600, np.int64)
    r.prolix(out, 1)                                                          # opens the device-side stack
    assert (out == px[1]).all()
    for clone in (copy.copy(r), copy.deepcopy(r), pickle.loads(pickle.dumps(r))):
        assert clone._stack is None
        clone.prolix(out, 2)
        assert (out == px[2]).all()
    del clone, r                                                              # two closes of one handle would crash here


def test_host_entry_points_share_the_arena_workspace(gpu, oracle):
    """trpx_encode_host registers its thread's workspace slot as clean; trpx_group_states_host / trpx_frame_offsets_host write an
    index / a walk's scratch into the same slot (api.hip: Arena).  Terse compress -> write() with the frame index -> compress
    the next stack: the second encode must not trust a scribbled workspace (status 0, oracle bytes, no 0.25 s timeout)."""
    import ctypes, time
    from trpx_amd import _lib
    L = _lib.lib()
    n, frames = 512 * 512, 6
    a = oracle.synth(np.uint16, 40, frames, n)
    want, sizes, _ = oracle.encode_stack(a)
    cap = frames * L.trpx_worst_case_bytes(_lib.U16, n, 12)
    out = np.empty(cap, dtype=np.uint8)
    total = ctypes.c_size_t(0)
    offs = np.zeros(frames + 1, dtype=np.uint64)
    pb = ctypes.c_uint32(0)

    def enc():
        t0 = time.time()
        _lib.check(L.trpx_encode_host(_lib.U16, a.ctypes.data, n, frames, 12, out.ctypes.data, cap, ctypes.byref(total),
                                      offs.ctypes.data, ctypes.byref(pb), 0))
        assert time.time() - t0 < 0.2, "a look-back wait ran into its timeout"
        assert out[: total.value].tobytes() == want.tobytes()

    enc(); enc()
    ng = L.trpx_group_count(n, 12)
    states = np.zeros(frames * ng, dtype=np.uint64)
    _lib.check(L.trpx_group_states_host(out.ctypes.data, total.value, offs.ctypes.data, n, frames, 12, 16, states.ctypes.data, 0))
    enc()
    got = np.zeros(frames + 1, dtype=np.uint64)
    _lib.check(L.trpx_frame_offsets_host(out.ctypes.data, total.value, n, frames, 12, 16, got.ctypes.data, 0))
    assert (got == offs).all()
    enc(); enc()


def test_two_host_threads_share_the_library(gpu, oracle):
    """Two host threads, each with its own stream, workspaces and data, encode and decode at the same time (ctypes releases
    the GIL for the length of a call).  What they share is the library: the encoder's register of clean workspaces (one
    mutex, encode_fused.hip -- a clearing launch skipped for the wrong workspace would mean a damaged stream or a look-back
    timeout) and, per thread, the host wrappers' arena, error text and profiler (thread_local, api.hip).  Every stack must be
    the one the thread's own data gives single-threaded -- byte for byte -- and decode back to it."""
    import threading
    import torch
    from trpx_amd import codec
    n, frames, rounds = 512 * 512, 64, 25
    data, expect = [], []
    for t in range(2):
        px = codec.synth(np.uint16, 1000 * t, frames, n, device=gpu)
        enc = encode(px, index=False)
        want, _ = oracle.encode(px[0].cpu().numpy())
        o = enc.frame_offsets.cpu().numpy()
        assert enc.stack()[: int(o[1])].cpu().numpy().tobytes() == want.tobytes()
        data.append(px)
        expect.append((enc.stack().clone(), enc.frame_offsets.clone()))
    assert not torch.equal(expect[0][0][:4096], expect[1][0][:4096])                     # (different data: cross-talk would show)
    small = [np.random.RandomState(7 + t).poisson(2.0, (4, 256 * 256)).astype(np.uint16) for t in range(2)]
    small_want = [np.concatenate([oracle.encode(f)[0] for f in s]) for s in small]
    failures, gate = [], threading.Barrier(2)

    def work(t):
        try:
            torch.cuda.set_device(gpu)
            s = torch.cuda.Stream(device=gpu)
            ws_e, ws_d = codec.Workspace(gpu), codec.Workspace(gpu)
            px, (stack, offs) = data[t], expect[t]
            cap = (frames * codec.worst_case_bytes(torch.uint16, n) + 15) // 16 * 16
            out = torch.empty(cap, dtype=torch.uint8, device=gpu)
            fo = torch.empty(frames + 1, dtype=torch.int64, device=gpu)
            st_e = torch.empty(8, dtype=torch.int32, device=gpu)
            st_d = torch.empty(8, dtype=torch.int32, device=gpu)
            back = torch.empty_like(px)
            gate.wait(timeout=60)
            with torch.cuda.stream(s):
                for r in range(rounds):
                    e = codec.encode(px, out=out, workspace=ws_e, frame_offsets=fo, status=st_e)
                    codec.decode(out, fo, n, frames, np.uint16, out=back, workspace=ws_d, status=st_d)
                    s.synchronize()
                    if int(st_e[0].item()) != 0 or int(st_d[0].item()) != 0:
                        failures.append((t, r, "status", int(st_e[0].item()), int(st_d[0].item())))
                    elif not (torch.equal(fo, offs) and torch.equal(out[: stack.numel()], stack)):
                        failures.append((t, r, "stream differs"))
                    elif not torch.equal(back.view(torch.int16), px.view(torch.int16)):
                        failures.append((t, r, "pixels differ"))
            for r in range(3):                                                            # the host wrappers: per-thread arena and stream
                got, ho, _ = host_encode(small[t])
                if got.tobytes() != small_want[t].tobytes():
                    failures.append((t, r, "host stream differs"))
                if not (host_decode(got, ho, 256 * 256, 4, np.uint16) == small[t]).all():
                    failures.append((t, r, "host pixels differ"))
        except Exception as ex:                                                           # (an assert in a thread would be lost)
            failures.append((t, "exception", repr(ex)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=240)
    assert not any(th.is_alive() for th in threads), "a thread did not come back"
    assert not failures, failures[:5]
