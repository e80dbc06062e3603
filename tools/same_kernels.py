#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel for kernel?  (CPU only: hipcc cross-compiles.)

    tools/same_kernels.py <tree_a> <tree_b> [--variants]

Every .hip unit of trpx_amd/csrc's OBJS is compiled to device assembly with the tree's own product flags (the compile lines are
the Makefile's, from `make -n`, with `--offload-device-only -S` in place of `-c`); with --variants also every (library, source,
flags) of the Makefile's variant libraries and the `noflag` objects.  The assembly is cut into functions by symbol, comments are
stripped, and what a pure source move changes is normalised: the `__hip_cuid_<hash>` symbol (it hashes the source), the function
index in the `.LBB<n>_<m>` / `.Lfunc_end<n>` labels, and the index of a string literal in its unit (`.str.<n>`, the printf formats
of diagnostic builds: the string itself stands in for its label).  A library's kernels are compared by symbol, whichever unit
holds them; a kernel that several units emit (templates of shared headers) counts once per distinct text.  The text is compared,
nothing is looked for in it.  Exit status 1 if a kernel differs or exists on one side only.
"""
import argparse
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def compile_lines(tree, variants):
    """[(library, stem, argv)] of the tree's Makefile: 'product' for OBJS, the library's name for a variant object."""
    csrc = os.path.join(tree, "trpx_amd", "csrc")
    targets = ["all"]
    if variants:
        db = subprocess.run(["make", "-pnq", "-C", csrc], capture_output=True, text=True).stdout
        libs = re.search(r"^VARIANT_LIBS :?= (.*)$", db, re.M).group(1).split()
        targets += ["noflag"] + ["../../tools/variants/libtrpx_%s.so" % lib for lib in libs]
    out = subprocess.run(["make", "-n", "-B", "-C", csrc] + targets, capture_output=True, text=True, check=True).stdout
    jobs = []
    for line in out.splitlines():
        m = re.search(r" -c (\S+)\.hip -o (\S+)\.o$", line)
        if not m:
            continue
        stem, obj = m.group(1), os.path.basename(m.group(2))
        lib = "product" if obj == stem else obj[len("trpx_"):-len(stem) - 1]
        argv = [a for a in line[:m.start()].split() if a not in ("-MMD", "-MP")]
        jobs.append((lib, stem, argv + ["--offload-device-only", "-S", stem + ".hip"]))
    return csrc, jobs


def functions(asm):
    """{symbol: text} of one assembly file: the function's body and, for a kernel, its descriptor."""
    asm = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", asm)
    asm = re.sub(r"\.LBB\d+_", ".LBB_", asm)
    asm = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", asm)
    strings = dict(re.findall(r"^(\.str(?:\.\d+)?):\n\s+\.asciz\s+(.*)$", asm, re.M))       # (printf formats of the diagnostic builds)
    asm = re.sub(r"\.str(?:\.\d+)?(?=@)", lambda m: ".str<%s>" % strings.get(m.group(0), m.group(0)).replace(";", "\\x3b"), asm)
    found, sym, desc, tail = collections.defaultdict(list), None, None, False
    for line in asm.splitlines():
        line = line.split(";")[0].rstrip()
        if not line:
            continue
        if tail and not re.match(r"\s+\.(size|set)\s", line):          # (the register counts follow the body as .set lines)
            sym, tail = None, False
        m = re.match(r"\s+\.type\s+(\S+),@function", line)
        if m:
            sym = m.group(1)
        m = re.match(r"\s+\.amdhsa_kernel\s+(\S+)", line)
        if m:
            desc = m.group(1)
        if sym or desc:
            found[sym or desc].append(line)
        if line.startswith(".Lfunc_end"):
            tail = True
        if line.strip() == ".end_amdhsa_kernel":
            desc = None
    return {s: "\n".join(t) for s, t in found.items()}


def kernels(tree, variants, out_dir):
    """{(library, symbol): [text, ...]} for every compile line of the tree."""
    csrc, jobs = compile_lines(tree, variants)

    def one(job):
        lib, stem, argv = job
        path = os.path.join(out_dir, "%s_%s.s" % (lib, stem))
        subprocess.run(argv + ["-o", path], cwd=csrc, check=True)
        with open(path) as f:
            return lib, functions(f.read())

    table = collections.defaultdict(list)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for lib, funcs in pool.map(one, jobs):
            for sym, text in funcs.items():
                table[(lib, sym)].append(text)
    return {k: sorted(set(v)) for k, v in table.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--variants", action="store_true", help="also every variant library of the Makefile, and `make noflag`")
    args = ap.parse_args()
    os.makedirs(os.path.join(HERE, "variants"), exist_ok=True)
    out = tempfile.mkdtemp(prefix="same_kernels_", dir=os.path.join(HERE, "variants"))
    sides = []
    for name, tree in (("a", args.tree_a), ("b", args.tree_b)):
        os.mkdir(os.path.join(out, name))
        sides.append(kernels(os.path.abspath(tree), args.variants, os.path.join(out, name)))
    a, b = sides
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for title, keys in (("only in " + args.tree_a, only_a), ("only in " + args.tree_b, only_b), ("differ", differ)):
        for lib, sym in keys:
            print("%s: %s: %s" % (title, lib, sym))
    libs = sorted({lib for lib, _ in a} | {lib for lib, _ in b})
    for lib in libs:
        print("%-14s %4d kernels compared" % (lib, sum(1 for k in set(a) & set(b) if k[0] == lib)))
    print("%d kernels compared in %d libraries: %d differ, %d + %d on one side only (assembly kept in %s)"
          % (len(set(a) & set(b)), len(libs), len(differ), len(only_a), len(only_b), out))
    return 1 if differ or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main())
