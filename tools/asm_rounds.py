"""Diagnostic (CPU only): the load rounds of one kernel in the compiled device code.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -Iinclude \
        -Idistributed-faas_amd/csrc distributed-faas_amd/csrc/faasbal_kernels.hip -o k.s
    python tools/asm_rounds.py k.s SYMBOL [--from N --to M] [--all]

Prints, with their line numbers inside the symbol, the global_load / s_load / s_waitcnt /
s_barrier lines, the labels and the branches of SYMBOL (--all: also LDS accesses and
global stores), so a role's path can be read off: loads that are separated by a
`s_waitcnt vmcnt` are dependent memory rounds.  A line "== round k: n loads" is
added wherever a vmcnt wait follows loads issued since the previous one.
"""
import argparse
import re
import sys

KEEP = re.compile(r"^\s*(global_load|buffer_load|flat_load|scratch_load|s_load|s_waitcnt|s_barrier|"
                  r"s_cbranch|s_branch|s_endpgm|s_setpc)")
MORE = re.compile(r"^\s*(ds_|global_store|global_atomic|s_memtime|s_memrealtime)")
LABEL = re.compile(r"^\.LBB\d+_\d+:")


def body(lines, sym):
    start = None
    for i, ln in enumerate(lines):
        if ln.startswith(sym + ":"):
            start = i + 1
            break
    if start is None:
        sys.exit("symbol not found: " + sym)
    out = []
    for ln in lines[start:]:
        if ln.startswith(".Lfunc_end"):
            break
        out.append(ln.rstrip("\n"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("symbol")
    ap.add_argument("--from", dest="lo", type=int, default=0, help="first line of the symbol to print")
    ap.add_argument("--to", dest="hi", type=int, default=1 << 30, help="last line of the symbol to print")
    ap.add_argument("--all", action="store_true", help="also LDS accesses, global stores and atomics, clock reads")
    args = ap.parse_args()
    with open(args.asm) as f:
        b = body(f.readlines(), args.symbol)
    pending, rnd = 0, 0
    for i, ln in enumerate(b):
        if i < args.lo or i > args.hi:
            continue
        code = ln.split(";")[0].rstrip()
        if LABEL.match(ln):
            print("%6d %s" % (i, code))
            continue
        if not (KEEP.match(code) or (args.all and MORE.match(code))):
            continue
        print("%6d %s" % (i, " ".join(code.split())))
        op = code.split()[0]
        if op.startswith(("global_load", "buffer_load", "flat_load")):
            pending += 1
        elif op == "s_waitcnt" and "vmcnt" in code and pending:
            rnd += 1
            print("       == round %d: %d loads" % (rnd, pending))
            pending = 0


if __name__ == "__main__":
    main()
