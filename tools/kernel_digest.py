#!/usr/bin/env python3
"""One digest per device kernel of a source tree: `python tools/kernel_digest.py [TREE] > digests.txt`.

Compiles every unit of TREE's flasht5_amd/build.py (its UNITS, with its FLAGS) to gfx950 assembly and prints, sorted,
`<sha256> <kernel symbol> <unit object>` for every kernel.  Two trees whose first two columns compare equal
(`cut -d' ' -f1,2 a.txt | diff - <(cut -d' ' -f1,2 b.txt)`) run the same device code, however the kernels are spread over
translation units -- the check behind a source clean-up or a re-cut of the units.  A kernel emitted by two units is an error.

A digest covers the kernel's instructions, its local labels and its .amdhsa_* resource directives; comments and other directives
are dropped.  Local labels (.LBB<n>_<k>, .Lfunc_end<n>, .Ltmp<n>, ...) carry the function's position in its unit, so their numbers
are replaced by the order in which they first appear within the kernel.
"""
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(?![0-9])")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_fat5_build", os.path.join(tree, "flasht5_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(build, unit, out_dir):
    src, obj, defs = unit
    out = os.path.join(out_dir, obj[:-2] + ".s")
    cmd = [build.HIPCC] + build.FLAGS + defs + ["--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {obj}:\n{r.stderr[-3000:]}")
    return obj, out


def kernels_of(path):
    """{kernel symbol: text to hash} of one assembly file"""
    lines = []
    for raw in open(path):
        s = raw.split(";", 1)[0].strip()
        if s:
            lines.append(s)
    names = {s.split()[1] for s in lines if s.startswith(".amdhsa_kernel ")}
    body, desc = {}, {}
    cur = in_desc = None
    for s in lines:
        if s.startswith(".amdhsa_kernel "):
            in_desc = s.split()[1]
            desc[in_desc] = []
        elif s == ".end_amdhsa_kernel":
            in_desc = None
        elif in_desc:
            desc[in_desc].append(s)
        elif s.endswith(":") and s[:-1] in names:
            cur = s[:-1]
            body[cur] = []
        elif cur and re.fullmatch(r"\.Lfunc_end\d+:", s):
            cur = None
        elif cur and (not s.startswith(".") or s.startswith(".L")):
            body[cur].append(s)
    out = {}
    for name in names:
        seen = {}

        def renumber(m, seen=seen):
            return ".L%s#%d" % (m.group(1), seen.setdefault(m.group(0), len(seen)))

        out[name] = "\n".join(LOCAL.sub(renumber, s) for s in body[name] + desc[name])
    return out


def main():
    tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
    build = load_build(tree)
    rows, owner = [], {}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as ex:
        for obj, path in ex.map(lambda u: assemble(build, u, tmp), build.UNITS):
            for name, text in kernels_of(path).items():
                if name in owner:
                    sys.exit(f"kernel {name} is emitted by both {owner[name]} and {obj}")
                owner[name] = obj
                rows.append((hashlib.sha256(text.encode()).hexdigest(), name, obj))
    for row in sorted(rows, key=lambda r: r[1]):
        print(*row)
    print(f"{len(rows)} kernels in {len(build.UNITS)} units", file=sys.stderr)


if __name__ == "__main__":
    main()
