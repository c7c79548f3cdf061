#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of the libraries, kernel by kernel.  Needs no GPU.

    python tools/compare_kernel_code.py OLD.so NEW.so [OLD2.so NEW2.so ...] [--out REPORT.txt]

Every code object of a library (kernel_resources.code_objects) is disassembled with llvm-objdump and split per symbol;
the `// address: bytes <sym+off>` comments are dropped.  Kernels (the symbols with a kernel descriptor) are matched by
their demangled name without the parameter list, so a kernel whose parameter types moved to another namespace is still
the same kernel.  Device functions the compiler left out of line are matched by content, since their names may change.
A verdict per symbol (the report lists identical kernels by template, with the number of instantiations):

    identical          the same instructions, line for line
    displacements      the same but for the literals of pc-relative addresses of other symbols (the s_add_u32 /
                       s_addc_u32 after an s_getpc_b64), which move with the layout of the code object
    different N        N lines differ

The report also says whether the two builds hold the same set of kernel names and the same resource rows
(kernel_resources.kernel_resources, every field).  Exit status 0 only if nothing differs."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402

OBJDUMP = os.path.join(kr.LLVM, "llvm-objdump")
LABEL = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
PCREL = re.compile(r"^(s_addc?_u32 \S+ \S+ )\S+$")


def _symbols(path):
    """{mangled name: [instruction lines]} of one code object, and the names that are kernels."""
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], capture_output=True, text=True,
                         check=True).stdout
    syms, cur = {}, None
    for line in txt.splitlines():
        m = LABEL.match(line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        line = " ".join(line.split("//")[0].split())
        if cur is not None and line:
            cur.append(line)
    for lines in syms.values():  # the padding up to the next symbol is layout, not code
        while lines and lines[-1].startswith(("s_nop", "s_code_end")):
            lines.pop()
    nm = subprocess.run([os.path.join(kr.LLVM, "llvm-readelf"), "--symbols", "--wide", path], capture_output=True, text=True,
                        check=True).stdout
    names = {l.split()[-1] for l in nm.splitlines() if l.split()}
    return syms, {n for n in syms if n + ".kd" in names}


def _masked(lines):
    """The lines with the literals of pc-relative address sums (up to 4 lines after an s_getpc_b64) blanked."""
    out, window = [], 0
    for l in lines:
        if l.startswith("s_getpc_b64"):
            window = 5
        m = PCREL.match(l.replace(",", "")) if window > 0 else None
        out.append(m.group(1) + "<disp>" if m else l)
        window -= 1
    return out


def library(so_path):
    """({kernel name: lines}, [lines of every out-of-line device function]) over all code objects of the library."""
    kernels, funcs = {}, []
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for i, co in enumerate(kr.code_objects(so_path)):
            paths.append(os.path.join(td, f"co{i}.o"))
            open(paths[-1], "wb").write(co)
        with ThreadPoolExecutor(max_workers=8) as ex:
            parts = list(ex.map(_symbols, paths))
    for syms, kern in parts:
        mangled = sorted(kern)
        for mn, dn in zip(mangled, kr._demangle(mangled)):
            kernels[dn] = syms[mn]
        funcs += [syms[n] for n in syms if n not in kern]
    return kernels, funcs


def compare(old_so, new_so, rows):
    ok = True
    rows.append(f"== {old_so} -> {new_so}")
    (ko, fo), (kn, fn) = library(old_so), library(new_so)
    counts = {"identical": 0, "displacements": 0, "different": 0}
    same = {}  # identical kernels, one row per template: [instantiations, lines]
    for name in sorted(set(ko) & set(kn)):
        a, b = ko[name], kn[name]
        if a == b:
            fam = same.setdefault(name.split("<")[0], [0, 0])
            fam[0], fam[1] = fam[0] + 1, fam[1] + len(b)
            counts["identical"] += 1
            continue
        elif _masked(a) == _masked(b):
            verdict = "displacements"
        else:
            n = sum(1 for d in difflib.unified_diff(_masked(a), _masked(b), lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            verdict = f"different {n}"
            ok = False
        counts[verdict.split()[0]] += 1
        rows.append(f"{name[:100]:100s} {len(b):7d} lines  {verdict}")
    rows += [f"{k + ' (' + str(n) + ' kernels)':100s} {lines:7d} lines  identical" for k, (n, lines) in sorted(same.items())]
    gone, new = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
    rows += [f"kernel only in the old build: {k}" for k in gone] + [f"kernel only in the new build: {k}" for k in new]
    rows.append(f"kernels: {len(kn)} ({counts['identical']} identical, {counts['displacements']} identical up to displacements, "
                f"{counts['different']} different); set of names {'unchanged' if not gone and not new else 'CHANGED'}")
    old_funcs = {tuple(_masked(f)) for f in fo}
    unmatched = [f for f in fn if tuple(_masked(f)) not in old_funcs]
    rows.append(f"out-of-line device functions: {len(fo)} old, {len(fn)} new, {len(unmatched)} of the new ones without an "
                f"old one of the same content")
    ro, rn = kr.kernel_resources(old_so), kr.kernel_resources(new_so)
    moved = sorted(k for k in set(ro) | set(rn) if ro.get(k) != rn.get(k))
    rows += [f"resource row differs: {k}: {ro.get(k)} -> {rn.get(k)}" for k in moved]
    rows.append(f"resource rows: {len(rn)}, {'all equal in every field' if not moved else str(len(moved)) + ' DIFFER'}")
    return ok and not gone and not new and not unmatched and not moved


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="OLD.so NEW.so pairs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if len(a.libs) % 2:
        ap.error("libraries come in pairs: OLD.so NEW.so")
    rows = ["# machine code of the kernels, old build against new build (tools/compare_kernel_code.py)"]
    good = all([compare(o, n, rows) for o, n in zip(a.libs[0::2], a.libs[1::2])])
    rows.append("verdict: " + ("no kernel differs" if good else "DIFFERENCES (see above)"))
    text = "\n".join(rows) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)
    sys.exit(0 if good else 1)
