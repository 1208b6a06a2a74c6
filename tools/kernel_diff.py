#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libsdfgrid.so without a GPU: for every kernel symbol the metadata
tests/test_abi.py reads (registers, spills, LDS, scratch, kernel-argument bytes) and the opcode multiset of its disassembly
(opcode plus the `nt` marker).  Reads the code objects with the LLVM binary tools only (tests/kernel_objects.py).

    python tools/kernel_diff.py OLD/libsdfgrid.so NEW/libsdfgrid.so [--pair OLD_SYMBOL=NEW_SYMBOL ...] [--new-ok]

--pair matches a kernel whose symbol changed with its predecessor.  --new-ok: a change that ADDS kernels -- those only in NEW are
listed with their metadata and are no failure (a kernel only in OLD still is).  The disassembler's "..." (how llvm-objdump prints
a run of zero bytes, e.g. the padding behind a kernel's last instruction) is no opcode and is not counted.
Exit status 1 if the kernel sets differ (after pairing),
if LDS / scratch / spills / kernel-argument bytes differ or VGPRs rose for any kernel, or if the counts of global_load* /
global_store* / ds_* opcodes differ; every other difference (SGPRs, other opcodes) is listed and left to the reader."""
import argparse
import ctypes
import os
import pathlib
import sys
import tempfile
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from kernel_objects import kernel_table, opcodes, unbundle  # noqa: E402

EQUAL = ("lds", "scratch", "vgpr_spill", "sgpr_spill", "kernarg")


def build_id(lib):
    f = ctypes.CDLL(os.path.abspath(lib)).sdfv_build_id
    f.restype = ctypes.c_char_p
    return f().decode()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--new-ok", action="store_true")
    args = ap.parse_args()
    renamed = dict(p.split("=", 1) for p in args.pair)
    with tempfile.TemporaryDirectory() as tmp:
        tables = []
        for k, lib in enumerate((args.old, args.new)):
            d = pathlib.Path(tmp) / str(k)
            d.mkdir()
            tables.append(kernel_table(unbundle(lib, d)))
        old, new = tables
        print(f"old: {args.old}  build id {build_id(args.old)}  {len(old)} kernels")
        print(f"new: {args.new}  build id {build_id(args.new)}  {len(new)} kernels")
        bad = False
        for o, n in renamed.items():
            print(f"paired by hand: {o}\n            -> {n}")
        only_old = sorted(k for k in old if renamed.get(k, k) not in new)
        only_new = sorted(set(new) - {renamed.get(k, k) for k in old})
        for k in only_old:
            print(f"ONLY IN OLD: {k}")
        for k in only_new:
            print(f"ONLY IN NEW: {k}" + ("  " + " ".join(f"{key} {new[k][key]}" for key in ("vgpr", "sgpr") + EQUAL) if args.new_ok else ""))
        bad = bad or bool(only_old) or (bool(only_new) and not args.new_ok)
        identical = differing = 0
        for name in sorted(old):
            if renamed.get(name, name) not in new:
                continue
            a, b = old[name], new[renamed.get(name, name)]
            oa, ob = (Counter(op for op in opcodes(k["co"], sym) if op != "...") for k, sym in ((a, name), (b, renamed.get(name, name))))
            notes = [f"{key} {a[key]} -> {b[key]}" for key in ("vgpr", "sgpr") + EQUAL if a[key] != b[key]]
            notes += [f"{op} {oa[op]} -> {ob[op]}" for op in sorted(set(oa) | set(ob)) if oa[op] != ob[op]]
            failed = any(a[key] != b[key] for key in EQUAL) or b["vgpr"] > a["vgpr"] or any(
                oa[op] != ob[op] for op in set(oa) | set(ob) if op.startswith(("global_load", "global_store", "ds_")))
            if notes:
                differing += 1
                print(("FAIL " if failed else "diff ") + name + ": " + "; ".join(notes))
            else:
                identical += 1
            bad = bad or failed
        print(f"{identical} kernels with equal metadata and opcode multisets, {differing} with a difference")
        print("RESULT: " + ("FAIL" if bad else "ok"))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
