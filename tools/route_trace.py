"""The launch sequence of every decode route, call by call -- what DESIGN.md 4.6 tabulates, read off the GPU.

Run (GPU box, library from $TRPX_LIB or the tree's):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/route_trace.py --out DIR
calls trpx_decode (with and without offsets), trpx_build_index, trpx_decode_indexed and trpx_decode_sum / _roi / _sparse / _dot
without an index once per stack under the selectors 0 .. 5 of trpx_set_decode_path.  Every call is preceded by one k_synth
launch, so the trace falls into one segment per call; the labels go to DIR/calls_<pid>.txt.  The many-frames rule's stacks run
as 4 frames under TRPX_SINGLE_PART=4,1048576 in a child process of their own (the rule is read when the library loads).

    python3 tools/route_trace.py --compare DIR_A DIR_B
prints, per call, the ordered (kernel, grid, workgroup) lists of two such runs where they differ, and exits 1 if any does."""
import argparse, csv, glob, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stacks(many):
    import numpy as np
    if many:      # frames of more than 32 K blocks kept whole: below and above the per-frame decoder's 2^26 bits
        return [("4x640^2 u16 whole", np.uint16, 4, 640, 640, "synth"), ("4x2048^2 u16 whole", np.uint16, 4, 2048, 2048, "synth")]
    return [("4x64^2 u16", np.uint16, 4, 64, 64, "synth"), ("4x65.63 u16", np.uint16, 4, 63, 65, "synth"),
            ("3x64^2 u16", np.uint16, 3, 64, 64, "synth"), ("8x512^2 u16", np.uint16, 8, 512, 512, "synth"),
            ("3x1030.1065 u16", np.uint16, 3, 1065, 1030, "synth"), ("3x1030.1065 i32", np.int32, 3, 1065, 1030, "synth"),
            ("3x1030.1065 u16 poisson3", np.uint16, 3, 1065, 1030, "poisson"),
            ("1x2048^2 u16", np.uint16, 1, 2048, 2048, "synth"), ("1x2048^2 i32", np.int32, 1, 2048, 2048, "synth"),
            ("1024x64^2 u16", np.uint16, 1024, 64, 64, "synth"), ("1023x64^2 u16", np.uint16, 1023, 64, 64, "synth"),
            ("1024x65.63 u16", np.uint16, 1024, 63, 65, "synth")]


def run(out_dir, many):
    import torch
    from trpx_amd import codec, workloads, _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    labels = []
    dot = torch.empty(1, dtype=torch.uint16, device=dev)

    def mark(label):                                          # one k_synth launch in front of the call
        labels.append(label)
        _lib.check(L.trpx_synth_fill(_lib.U16, 0, 0, 1, 1, dot.data_ptr(), codec._stream_ptr(dot)))

    ws = codec.Workspace(dev)
    for name, dt, f, h, w, kind in stacks(many):
        n = h * w
        if kind == "synth":
            labels.append(f"build {name}")                    # (codec.synth is a k_synth launch itself)
            px = codec.synth(dt, 0, f, n, device=dev)
        else:
            mark(f"build {name}")
            px = workloads.poisson_u16(3.0, 0, f, n, device=dev)
        enc = codec.encode(px)
        enc.check()
        terse, offs = enc.stack(), enc.frame_offsets
        box = torch.tensor([[0, 0, 0]], dtype=torch.int32, device=dev)
        high = 1 << (14 if px.dtype == torch.uint16 else 28)
        ones = torch.ones((1, n), dtype=torch.int32, device=dev)

        def decoded(label, **kw):
            mark(label)
            back, st = codec.decode(terse, kw.pop("offsets", offs), n, f, kw.pop("dtype", dt), workspace=ws, **kw)
            want = px if back.dtype == px.dtype else px.to(back.dtype)
            assert int(st[0].item()) == 0 and torch.equal(back.view(torch.uint8), want.view(torch.uint8)), label

        for sel in range(6):
            _lib.check(L.trpx_set_decode_path(sel))
            tag = f"{name} selector {sel}: "
            decoded(tag + "decode")
            decoded(tag + "decode, no offsets", offsets=None)
            mark(tag + "build_index")
            index = codec.build_index(terse, offs, n, f, dt)
            decoded(tag + "decode_indexed", index=index)
            mark(tag + "decode_sum")
            _, st = codec.decode_sum(terse, offs, n, f, dt, f, workspace=ws)
            assert int(st[0].item()) == 0, tag
            mark(tag + "decode_roi")
            _, st = codec.decode_roi(terse, offs, n, f, dt, w, box, (8, 8), workspace=ws)
            assert int(st[0].item()) == 0, tag
            mark(tag + "decode_sparse")
            _, _, _, st = codec.decode_sparse(terse, offs, n, f, dt, high, capacity=4096, workspace=ws)
            assert int(st[0].item()) in (_lib.OK, _lib.ERR_CAPACITY), tag
            mark(tag + "decode_dot")
            _, st = codec.decode_dot(terse, offs, n, f, dt, ones, workspace=ws)
            assert int(st[0].item()) == 0, tag
        _lib.check(L.trpx_set_decode_path(0))
        if name == "4x64^2 u16":                              # the routes outside the tuned decoders
            decoded(name + ": decode into int64", dtype=torch.int64, stream_signed=False)
            decoded(name + ": decode into int64, no offsets", dtype=torch.int64, stream_signed=False, offsets=None)
            enc13 = codec.encode(px, block=13)
            enc13.check()
            for o in (enc13.frame_offsets, None):
                mark(name + ": block 13" + ("" if o is not None else ", no offsets"))
                back, st = codec.decode(enc13.stack(), o, n, f, dt, workspace=ws, block=13)
                assert int(st[0].item()) == 0 and torch.equal(back.view(torch.uint8), px.view(torch.uint8))
        del px, enc
    torch.cuda.synchronize()
    with open(os.path.join(out_dir, f"calls_{os.getpid()}.txt"), "w") as fh:
        fh.write("\n".join(labels) + "\n")
    print(f"route_trace: {len(labels)} segments ({'many-frames rule' if many else 'built-in rule'})", flush=True)


def segments(d):
    """{label: [(kernel, grid, workgroup), ...]} of one run's directory."""
    out = {}
    for calls in sorted(glob.glob(os.path.join(d, "calls_*.txt"))):
        pid = os.path.basename(calls)[6:-4]
        traces = [p for p in glob.glob(os.path.join(d, "**", f"{pid}_kernel_trace.csv"), recursive=True)]
        assert len(traces) == 1, (calls, traces)
        rows = list(csv.DictReader(open(traces[0])))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        dims = lambda r, what: tuple(int(r[f"{what}_{a}"]) for a in "XYZ")
        segs = []
        for r in rows:
            k = r["Kernel_Name"]
            if "trpx::" not in k:
                continue                                       # (torch's own kernels: the checks, the Poisson stack)
            if "k_synth" in k:
                segs.append([])
            elif segs:
                segs[-1].append((k, dims(r, "Grid_Size"), dims(r, "Workgroup_Size")))
        labels = open(calls).read().splitlines()
        assert len(labels) == len(segs), (calls, len(labels), len(segs))
        for label, s in zip(labels, segs):
            assert label not in out, label
            out[label] = s
    return out


def compare(a, b):
    sa, sb = segments(a), segments(b)
    bad = [k for k in sa if sa[k] != sb.get(k)] + [k for k in sb if k not in sa]
    for k in bad:
        print("DIFFERS", k)
        for tag, s in (("  a", sa.get(k)), ("  b", sb.get(k))):
            for e in s or [("(no such call)",)]:
                print(tag, *e)
    launches = sum(len(s) for s in sa.values())
    print(f"route_trace: {len(sa)} calls, {launches} launches in {a}; {len(bad)} calls differ from {b}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--many-frames", action="store_true", help="(the child process: TRPX_SINGLE_PART is set)")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    ap.add_argument("--print", metavar="DIR", help="every call's launches of one run")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.print:
        for label, s in segments(a.print).items():
            print(label)
            for e in s:
                print("   ", *e)
        sys.exit(0)
    os.makedirs(a.out, exist_ok=True)
    if not a.many_frames:      # first, and on its own: this process has not touched the GPU yet
        env = dict(os.environ, TRPX_SINGLE_PART="4,1048576")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--out", a.out, "--many-frames"], env=env, check=True, timeout=300)
    run(a.out, a.many_frames)
