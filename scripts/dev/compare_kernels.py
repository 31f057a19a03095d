#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of a library, per kernel symbol:

    python scripts/dev/compare_kernels.py [--rename PATTERN REPL]... OLD.so NEW.so

For every kernel of the two libraries' code objects: the set of names, the kernel's metadata entry
(registers, LDS, scratch, spills, kernarg layout: the whole amdhsa.kernels record) and its machine
code.  Code that differs byte for byte is compared again as disassembly with the addresses dropped
and the literal of each pc-relative address pair (s_getpc_b64 ... s_add_u32 / s_addc_u32) masked: a
kernel that differs only there addresses the same constant table at another distance because the
object's layout moved.  Prints counts per kernel family and every difference; exit status 1 if a
kernel was added, removed or differs otherwise.  A refactor of host code must print zero differences.
--rename applies re.sub(PATTERN, REPL) to OLD's demangled names first, for a refactor that changed a
kernel's template parameter list; the metadata records are then compared without their .name and
.symbol fields (the mangled names), which differ for a renamed kernel by construction.
"""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
from test_kernel_resources import LLVM, code_objects  # noqa: E402


def _elf_functions(path):
    """{symbol: code bytes} of the FUNC symbols of an ELF64 little-endian object."""
    blob = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ != 2:   # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for j in range(size // entsize):
            name, info, _, shndx, value, fsize = struct.unpack_from("<IBBHQQ", blob, off + j * entsize)
            if info & 0xF != 2 or not fsize or not 0 < shndx < shnum:   # STT_FUNC, defined
                continue
            sec = secs[shndx]
            start = sec[4] + value - sec[3]
            out[blob[stroff + name:blob.index(b"\0", stroff + name)].decode()] = blob[start:start + fsize]
    return out


def _disassembly(co):
    """{symbol: [instruction text]} with addresses, encodings and pc-relative literals dropped."""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True,
                          text=True, check=True).stdout
    out, cur, getpc = {}, None, 0
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins:
            continue
        if ins.startswith("s_getpc_b64"):
            getpc = 8          # the address pair follows within a few instructions
        elif getpc and re.match(r"s_addc?_u32 .*, (0x[0-9a-f]+|-?\d+)$", ins):
            ins = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", ins)
        getpc = max(getpc - 1, 0)
        cur.append(ins)
    return out


def kernels(lib, drop_names=False):
    """{demangled name: (metadata record, code bytes, normalised disassembly)}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            code, dis = _elf_functions(co), _disassembly(co)
            for ent in notes.split("  - .agpr_count:")[1:]:
                sym = re.search(r"\.name:\s+(\S+)", ent).group(1)
                ent = ent.split("amdhsa.target:")[0]
                if drop_names:   # a renamed kernel's record differs in its own mangled names by construction
                    ent = re.sub(r"\.(name|symbol):\s+\S+", "", ent)
                out[sym] = (ent, code[sym], dis.get(sym, []))
    syms = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d: out[s] for s, d in zip(syms, dem)}


def family(name):
    return name.replace("(anonymous namespace)::", "").split("<")[0].replace("void ", "").split("(")[0].strip()


def main():
    renames = []
    while len(sys.argv) > 3 and sys.argv[1] == "--rename":
        renames.append(sys.argv[2:4])
        del sys.argv[1:4]
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1], bool(renames)), kernels(sys.argv[2], bool(renames))
    for pat, repl in renames:
        old = {re.sub(pat, repl, n): v for n, v in old.items()}
    counts = collections.Counter(family(n) for n in new)
    bad, pcrel = [], []
    for n in sorted(set(old) - set(new)):
        bad.append(f"removed: {n}")
    for n in sorted(set(new) - set(old)):
        bad.append(f"added: {n}")
    for n in sorted(set(old) & set(new)):
        (mo, co, do), (mn, cn, dn) = old[n], new[n]
        if mo != mn:
            bad.append(f"metadata differs: {n}")
        if co != cn:
            (pcrel if do == dn and len(co) == len(cn) else bad).append(f"code differs: {n}")
    print(f"old: {sys.argv[1]}: {len(old)} kernels, {sum(len(v[1]) for v in old.values())} bytes of code")
    print(f"new: {sys.argv[2]}: {len(new)} kernels, {sum(len(v[1]) for v in new.values())} bytes of code")
    for fam, c in sorted(counts.items()):
        print(f"  {c:5d}  {fam}")
    print(f"added / removed / differing kernels: {len(bad)}")
    for b in bad:
        print("  " + b)
    print(f"kernels that differ only in a pc-relative literal: {len(pcrel)}")
    for b in pcrel:
        print("  " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
