"""The check of legged_gym_amd/sim/abi.py against include/lgx.h (tests/test_abi_host.py).

`mismatches(structs, constants, sigs)` generates a C++17 program from the three tables, compiles it
against the header alone ($CXX, else c++; nothing is linked: the prototypes are only named inside
decltype), runs it and compares what it prints with the ctypes side:
  structs    sizeof, and offsetof / size of every field the bindings name (a field the header does
             not have is a compile error)
  constants  the value of every identifier
  functions  the class of the return type and of every parameter: void, ptr, i32, u32, i64, u64,
             f32, f64 (an enum is i32, size_t goes by its size, char* is a pointer)
and, from the header text, that the tables leave out no structure and no function.  It returns the
differences as messages that name the struct, field, constant or function; none means the mirror is
exact.  The probe's lines are sorted, so tables that name the same things compile once per process.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgx.h")

PRELUDE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
template <class T> constexpr const char* cls() {
  if constexpr (std::is_void_v<T>) return "void";
  else if constexpr (std::is_pointer_v<T>) return "ptr";
  else if constexpr (std::is_enum_v<T>) return "i32";
  else if constexpr (std::is_floating_point_v<T>) return sizeof(T) == 4 ? "f32" : sizeof(T) == 8 ? "f64" : "other";
  else if constexpr (std::is_integral_v<T> && (sizeof(T) == 4 || sizeof(T) == 8))
    return std::is_signed_v<T> ? (sizeof(T) == 4 ? "i32" : "i64") : (sizeof(T) == 4 ? "u32" : "u64");
  else return "other";
}
template <class R, class... A> void sig(const char* name, R (*)(A...)) {
  std::printf("F %s %s", name, cls<R>());
  ((std::printf(" %s", cls<A>())), ...);
  std::printf("\n");
}
"""


def header_text(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def header_functions(header=HEADER):
    return sorted(set(re.findall(r"\b(lgx_[a-z0-9_]+)\s*\(", header_text(header))))


def header_structs(header=HEADER):
    """The structures with a body (lgx_sim and lgx_comm are opaque: no `{`)."""
    return sorted(set(re.findall(r"typedef\s+struct\s+(lgx_[a-z0-9_]+)\s*\{", header_text(header))))


def probe_source(structs, constants, sigs, header=HEADER):
    lines = []
    for cls, cname in structs:
        lines.append(f'std::printf("S {cname} %zu\\n", sizeof({cname}));')
        for field in cls._fields_:
            f = field[0]
            lines.append(f'std::printf("M {cname} {f} %zu %zu\\n", offsetof({cname}, {f}), sizeof({cname}::{f}));')
    for ident in constants:
        lines.append(f'std::printf("C {ident} %lld\\n", (long long)({ident}));')
    for name in sigs:
        lines.append(f'sig("lgx_{name}", static_cast<decltype(&lgx_{name})>(nullptr));')
    body = "\n  ".join(sorted(set(lines)))
    return f'#include "{os.path.abspath(header)}"\n{PRELUDE}\nint main() {{\n  {body}\n  return 0;\n}}\n'


@functools.lru_cache(maxsize=None)
def run_probe(source):
    """Compile and run one probe: ({struct: size}, {(struct, field): (offset, size)}, {ident: value},
    {function: [return class, parameter classes...]}), or the compiler's message as a string."""
    cxx = os.environ.get("CXX") or "c++"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "abi_probe.cpp"), os.path.join(tmp, "abi_probe")
        with open(src, "w") as f:
            f.write(source)
        cc = subprocess.run([cxx, "-std=c++17", "-O0", "-w", "-o", exe, src], capture_output=True, text=True)
        if cc.returncode != 0:
            return cc.stderr
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    sizes, members, values, fns = {}, {}, {}, {}
    for line in out.splitlines():
        kind, *w = line.split()
        if kind == "S":
            sizes[w[0]] = int(w[1])
        elif kind == "M":
            members[w[0], w[1]] = (int(w[2]), int(w[3]))
        elif kind == "C":
            values[w[0]] = int(w[1])
        else:
            fns[w[0]] = w[1:]
    return sizes, members, values, fns


def ctype_class(t):
    """The probe's type class of a ctypes restype / argtype."""
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    code = getattr(t, "_type_", None) if issubclass(t, C._SimpleCData) else None
    if code in ("f", "d"):
        return {"f": "f32", "d": "f64"}[code]
    if isinstance(code, str) and code in "ilqILQ" and C.sizeof(t) in (4, 8):
        return ("i" if code in "ilq" else "u") + str(8 * C.sizeof(t))
    return "other"


def mismatches(structs, constants, sigs, header=HEADER, module=None):
    """Every difference between the three tables and the header, as messages; `module`: also require
    that `structs` lists every ctypes.Structure the module defines."""
    errs = []
    listed = [cname for _, cname in structs]
    for cname in header_structs(header):
        if cname not in listed:
            errs.append(f"{cname}: a structure of lgx.h that STRUCTS does not list")
    for cname in listed:
        if cname not in header_structs(header):
            errs.append(f"{cname}: listed in STRUCTS, but lgx.h defines no such structure")
    if module is not None:
        for name, obj in vars(module).items():
            if isinstance(obj, type) and issubclass(obj, C.Structure) and obj.__module__ == module.__name__ \
                    and name not in [cls.__name__ for cls, _ in structs]:
                errs.append(f"{name}: a ctypes.Structure of the bindings that STRUCTS does not list")
    mine, theirs = sorted(f"lgx_{n}" for n in sigs), header_functions(header)
    errs += [f"{fn}: declared in lgx.h, not in SIGS" for fn in theirs if fn not in mine]
    errs += [f"{fn}: in SIGS, not declared in lgx.h" for fn in mine if fn not in theirs]
    if errs:
        return errs   # the probe below would not compile, or would prove less than it claims
    res = run_probe(probe_source(structs, constants, sigs, header))
    if isinstance(res, str):
        return [f"the probe does not compile against lgx.h:\n{res}"]
    sizes, members, values, fns = res
    for cls, cname in structs:
        if C.sizeof(cls) != sizes[cname]:
            errs.append(f"{cname}: sizeof {C.sizeof(cls)} in the bindings ({cls.__name__}), {sizes[cname]} in lgx.h")
        for field in cls._fields_:
            d = getattr(cls, field[0])
            if (d.offset, d.size) != members[cname, field[0]]:
                errs.append(f"{cname}.{field[0]}: (offset, size) {(d.offset, d.size)} in the bindings "
                            f"({cls.__name__}), {members[cname, field[0]]} in lgx.h")
    for ident, value in constants.items():
        if value != values[ident]:
            errs.append(f"{ident}: {value} in the bindings, {values[ident]} in lgx.h")
    for name, (res_t, arg_ts) in sigs.items():
        got = [ctype_class(res_t)] + [ctype_class(t) for t in arg_ts]
        want = fns[f"lgx_{name}"]
        if got != want:
            errs.append(f"lgx_{name}: (return, arguments) {' '.join(got)} in the bindings, {' '.join(want)} in lgx.h")
    return errs
