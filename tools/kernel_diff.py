"""Device code of two builds, kernel by kernel.  No GPU needed.

    python tools/kernel_diff.py BUILD_DIR_A BUILD_DIR_B        (two copies of dropoutdecoding_amd/build)

For every object file of either directory: the gfx950 code object is unbundled (llvm-objdump --offloading, as build.packed_fp32_ops
does), its function symbols and their bytes are read (llvm-readelf), and the tool prints the functions only in A, only in B, and in both
with different bytes.  Names and bytes only: nothing is disassembled.  Exit code 1 if B has a function A lacks or a common one differs —
what a refactor that must not change device code may not do (the partner of engine_digest.py, which compares what the code computes).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def _run(tool, *args, cwd=None, stdin=None):
    r = subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, input=stdin, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{tool} {' '.join(args)}: rc {r.returncode}: {r.stderr[-300:]}")
    return r.stdout


def device_functions(obj_path: str) -> dict:
    """{mangled name: code bytes} of the functions in the gfx950 code object(s) bundled in a host object; {} if it has no device code."""
    d = tempfile.mkdtemp(prefix="ddkd")
    try:
        shutil.copy(obj_path, os.path.join(d, "x.o"))
        _run("llvm-objdump", "--offloading", "x.o", cwd=d)
        out = {}
        for f in sorted(os.listdir(d)):
            if "amdgcn" not in f:
                continue
            path = os.path.join(d, f)
            data = open(path, "rb").read()
            sections = {}                                   # index -> (address, file offset, type)
            for ln in _run("llvm-readelf", "-S", "--wide", path).splitlines():
                p = ln.replace("[", " ").replace("]", " ").split()
                if len(p) >= 6 and p[0].isdigit() and p[0] != "0":
                    sections[int(p[0])] = (int(p[3], 16), int(p[4], 16), p[2])
            for ln in _run("llvm-readelf", "-s", "--wide", path).splitlines():
                p = ln.split()
                if len(p) == 8 and p[3] == "FUNC" and p[6].isdigit():
                    addr, off, typ = sections[int(p[6])]
                    if typ != "PROGBITS":
                        continue
                    start, size = off + int(p[1], 16) - addr, int(p[2], 0)
                    out[p[7]] = data[start:start + size]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def demangle(names):
    """{mangled: readable}; the mangled names themselves where no demangler is installed."""
    names = list(names)
    tool = next((t for t in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if not names or tool is None:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, timeout=600)
    out = r.stdout.splitlines()
    return dict(zip(names, out)) if r.returncode == 0 and len(out) == len(names) else {n: n for n in names}


def main(dir_a: str, dir_b: str) -> int:
    objs = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    bad = 0
    for o in sorted(objs(dir_a) | objs(dir_b)):
        fa = device_functions(os.path.join(dir_a, o)) if o in objs(dir_a) else {}
        fb = device_functions(os.path.join(dir_b, o)) if o in objs(dir_b) else {}
        only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
        differ = sorted(n for n in set(fa) & set(fb) if fa[n] != fb[n])
        same = len(set(fa) & set(fb)) - len(differ)
        print(f"{o}: {len(fa)} / {len(fb)} functions, {same} identical, {len(only_a)} only in A, {len(only_b)} only in B, {len(differ)} differ")
        names = demangle(only_a + only_b + differ)
        for title, group in (("only in A", only_a), ("only in B", only_b), ("bytes differ", differ)):
            for n in sorted(group, key=lambda n: names[n]):
                print(f"  {title}: {names[n]}")
        bad += len(only_b) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
