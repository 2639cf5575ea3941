#!/usr/bin/env python3
"""Compare the machine code of named kernels between two builds of one object file or library.

    python tools/kernel_code_diff.py OLD NEW KERNEL [KERNEL ...]
    python tools/kernel_code_diff.py --all OLD NEW

OLD and NEW are host objects or shared libraries built by hipcc for one GPU architecture.  Their
device code objects are unbundled, disassembled (llvm-objdump -d) and the listed kernels compared
instruction by instruction: the text of every instruction with its operands (branch operands are
relative offsets), without addresses and encodings.  --all compares every kernel (every function with
a kernel descriptor, by its full signature) found in either input, so one present in only one of
them is reported as missing in the other.  Exit status 0 when every kernel is the same code in both, 1 otherwise.
Needs no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")


def objdump(tmp, co, *flags):
    return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), *flags, "-C", os.path.join(tmp, co)], text=True)


def functions(listing):
    """demangled function signature -> [instruction text].  The text is what stands before the
    `// address: encoding` comment; branch operands are relative offsets."""
    out, name = {}, None
    for line in listing.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:", line)
        if name is not None and m:
            out[name].append(m.group(1))
    return out


def kernels(path, tmp, tag):
    """kernel signature (demangled) -> [instruction text] over every code object of `path`: an object
    file holds one, a linked library one per translation unit.  A kernel is a function whose
    descriptor (<name>.kd) is in the symbol table."""
    # llvm-objdump --offloading writes every bundle of the fat binary next to the (linked) input
    os.symlink(os.path.abspath(path), os.path.join(tmp, tag))
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", tag], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    cos = sorted(f for f in os.listdir(tmp) if f.startswith(tag + ".") and f.endswith(ARCH))
    if not cos:
        raise SystemExit(f"{path}: no {ARCH} code object found")
    out = {}
    for co in cos:
        code = functions(objdump(tmp, co, "-d"))
        for m in re.finditer(r"^[0-9a-f]+ .*\t[0-9a-f]+ (?:\.[a-z]+ )?(.+) \(\.kd\)$", objdump(tmp, co, "-t"), re.M):
            if m.group(1) in out:
                raise SystemExit(f"{path}: two kernels with the signature {m.group(1)}")
            out[m.group(1)] = code[m.group(1)]
    return out


def main(argv):
    every = len(argv) > 1 and argv[1] == "--all"
    if every:
        del argv[1]
    if len(argv) < 4 - every or (every and len(argv) > 3):
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(argv[1], tmp, "old"), kernels(argv[2], tmp, "new")
    if every:
        pairs = [(k, k) for k in sorted(old.keys() | new.keys())]
    else:   # by name: the signature up to its argument list
        found = {k: [s for s in sorted(old.keys() | new.keys()) if s.split("(")[0] == k] for k in argv[3:]}
        pairs = [(k, s) for k in argv[3:] for s in found[k] or [k]]
    bad = 0
    for k, sig in pairs:
        a, b = old.get(sig), new.get(sig)
        if a is None or b is None:
            print(f"{k}: missing in {'OLD and NEW' if a is None and b is None else 'OLD' if a is None else 'NEW'}")
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
