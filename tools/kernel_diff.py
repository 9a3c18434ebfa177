#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same code?  (The proof a refactor owes: host only, no GPU.)

    python tools/kernel_diff.py old/liblav_amd.so new/liblav_amd.so

Every code object of both libraries is disassembled; functions are compared by mangled name, instruction for instruction, with what
is positional removed: addresses and encodings (the comment behind every instruction) and the literals of pc-relative address
arithmetic (the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64), the zero fill behind a function's last instruction (it depends
on which function the compiler emitted next: host code that names the kernels in another order moves it).  The kernels' register, scratch and LDS figures are compared
too.  Prints the kernels only one side has and the ones that differ; exit status 1 if a kernel of the new library differs or is new.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(lib):
    """{mangled name: (instructions, figures)} over all gfx950 code objects of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for o in sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950"))):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], check=True, stdout=subprocess.PIPE, text=True).stdout
            figs = {}
            for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
                blk = ".agpr_count" + blk
                figs[re.search(r"\.name:\s+(\S+)", blk).group(1)] = tuple(int(re.search(re.escape(f) + r":\s+(\d+)", blk).group(1)) for f in FIGURES)
            asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", o], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M):
                name, body, pcrel = m.group(1), [], 0
                for ln in m.group(2).splitlines():
                    ins = ln.split("//")[0].strip()
                    if not ins:
                        continue
                    if ins.startswith("s_getpc_b64"):
                        pcrel = 2
                    elif pcrel and re.match(r"s_addc?_u32 ", ins):
                        ins, pcrel = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "PCREL", ins), pcrel - 1
                    body.append(ins)
                while body and body[-1] == "...":   # the zero fill up to the next function's alignment: what follows the kernel, not the kernel
                    body.pop()
                assert name not in out, f"{name} is defined in two code objects"
                out[name] = (body, figs.get(name))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    print(f"{len(old)} functions in {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes), {len(new)} in {sys.argv[2]} ({os.path.getsize(sys.argv[2])} bytes), "
          f"{len(set(old) & set(new)) - len(differ)} identical ({sum(len(new[n][0]) for n in set(old) & set(new))} instructions; {', '.join(f[1:] for f in FIGURES)} "
          f"of {sum(new[n][1] is not None for n in new)} kernels)")
    for title, names in (("only in the old library", gone), ("only in the new library", added), ("DIFFERENT", differ)):
        for n in names:
            print(f"  {title}: {n}")
    for n in differ:
        a, b = old[n], new[n]
        first = next((i for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y), min(len(a[0]), len(b[0])))
        print(f"  {n}: {len(a[0])} -> {len(b[0])} instructions, first difference at {first}; figures {a[1]} -> {b[1]}")
    return 1 if added or differ else 0


if __name__ == "__main__":
    sys.exit(main())
