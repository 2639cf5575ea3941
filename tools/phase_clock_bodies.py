"""Summarise the "physics bodies:" lines of a phase-clock build (tools/phase_clock.sh; with
CLK_EXTRA=-DLGX_PHASE_CLOCK_ALL one line per workgroup and launch): per contact loop of
lgx_physics_kernel the executed bodies per launch - mean, maximum and histogram over the lines.
Usage: LGX_LIB_PATH=tools/_tmp/clock/liblgx.so python tools/phys_bench.py ... | python tools/phase_clock_bodies.py
       python tools/phase_clock_bodies.py LOG"""
import collections
import re
import sys


def main(stream):
    rows = [tuple(map(int, m.groups())) for m in
            re.finditer(r"physics bodies: b=\d+ pass0=(\d+) pass1=(\d+) classify=(\d+) report=(\d+)", stream.read())]
    print(f"{len(rows)} launch records")
    for i, name in enumerate(("pass-0 assembly", "pass-1 assembly", "classification", "force report")):
        xs = [r[i] for r in rows]
        if xs:
            print(f"{name}: mean {sum(xs) / len(xs):.2f} per launch, max {max(xs)}, "
                  f"histogram {sorted(collections.Counter(xs).items())}")


if __name__ == "__main__":
    main(open(sys.argv[1]) if len(sys.argv) > 1 else sys.stdin)
