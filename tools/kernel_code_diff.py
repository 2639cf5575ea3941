#!/usr/bin/env python3
"""Compare the machine code of named kernels between two builds of one object file or library.

    python tools/kernel_code_diff.py OLD NEW KERNEL [KERNEL ...]

OLD and NEW are host objects or shared libraries built by hipcc for one GPU architecture.  Their
device code objects are unbundled, disassembled (llvm-objdump -d) and the listed kernels compared
instruction by instruction: the text of every instruction with its operands (branch operands are
relative offsets), without addresses and encodings.  Exit status 0 when every kernel
is the same code in both, 1 otherwise.  Needs no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")


def disassemble(path, tmp, tag):
    # llvm-objdump --offloading writes every bundle of the fat binary next to the (linked) input
    os.symlink(os.path.abspath(path), os.path.join(tmp, tag))
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", tag], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    cos = sorted(f for f in os.listdir(tmp) if f.startswith(tag + ".") and f.endswith(ARCH))
    if not cos:
        raise SystemExit(f"{path}: no {ARCH} code object found")
    # an object file holds one code object, a linked library one per translation unit
    return "\n".join(subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", os.path.join(tmp, co)],
                                             text=True) for co in cos)


def kernels(listing):
    """kernel name (demangled, without its argument list) -> [instruction text].  The text is what
    stands before the `// address: encoding` comment; branch operands are relative offsets."""
    out, name = {}, None
    for line in listing.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1).split("(")[0]
            out[name] = []
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:", line)
        if name is not None and m:
            out[name].append(m.group(1))
    return out


def main(argv):
    if len(argv) < 4:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(disassemble(argv[1], tmp, "old")), kernels(disassemble(argv[2], tmp, "new"))
    bad = 0
    for k in argv[3:]:
        a, b = old.get(k), new.get(k)
        if a is None or b is None:
            print(f"{k}: missing in {'OLD' if a is None else 'NEW'}")
            bad += 1
        elif a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"{k}: DIFFERENT ({len(a)} vs {len(b)} instructions, first difference at {first})")
            bad += 1
        else:
            print(f"{k}: same code, {len(a)} instructions")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
