#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libsdfgrid.so without a GPU: for every kernel symbol the metadata
tests/test_abi.py reads (registers, spills, LDS, scratch, kernel-argument bytes) and the opcode multiset of its disassembly
(opcode plus the `nt` marker).  Reads the code objects with the LLVM binary tools only (tests/kernel_objects.py).

    python tools/kernel_diff.py OLD/libsdfgrid.so NEW/libsdfgrid.so [--pair OLD_SYMBOL=NEW_SYMBOL ...] [--new-ok]
    python tools/kernel_diff.py --dump-compiled DIR [--tree ROOT]      # the kernels sdfv_program_compile builds, as DIR/<program>.co
    python tools/kernel_diff.py OLD_DIR/demo3.co NEW_DIR/demo3.co      # ... and two of those compared the same way

An argument that is no .so is read as a bare gfx950 code object.  --dump-compiled: every program of PROGRAMS in
tests/test_program_compile_mesh_cpu.py compiled with all four routes for gfx950 (no device needed) by the library of the source
tree ROOT (default: this one), compiled_code() of each written to DIR.

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
from kernel_objects import bare_code_object, kernel_table, opcodes, unbundle  # noqa: E402

EQUAL = ("lds", "scratch", "vgpr_spill", "sgpr_spill", "kernarg")


def build_id(lib):
    f = ctypes.CDLL(os.path.abspath(lib)).sdfv_build_id
    f.restype = ctypes.c_char_p
    return f().decode()


def code_objects_of(path, tmp):
    """unbundle() of a library, or the one bare code object `path` is."""
    return unbundle(path, tmp) if path.endswith(".so") else bare_code_object(path)


def dump_compiled(out_dir, tree):
    sys.path.insert(0, tree)
    import importlib
    import program_compile_cases as CC
    from test_program_compile_cpu import builders
    from test_program_compile_mesh_cpu import PROGRAMS
    PM = importlib.import_module("sdf-viewer_amd.program")
    b = dict(builders(PM))
    b.update(CC.folding_programs(PM))
    os.makedirs(out_dir, exist_ok=True)
    for name in PROGRAMS:
        c = b[name].build().compile(PM.FILL | PM.POINTS | PM.MARCH | PM.MESH, arch="gfx950")
        pathlib.Path(out_dir, name + ".co").write_bytes(c.compiled_code())
    print(f"{len(PROGRAMS)} code objects in {out_dir} (library of {tree})")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--dump-compiled", metavar="DIR")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--new-ok", action="store_true")
    args = ap.parse_args()
    if args.dump_compiled:
        return dump_compiled(args.dump_compiled, os.path.abspath(args.tree))
    renamed = dict(p.split("=", 1) for p in args.pair)
    with tempfile.TemporaryDirectory() as tmp:
        tables = []
        for k, lib in enumerate((args.old, args.new)):
            d = pathlib.Path(tmp) / str(k)
            d.mkdir()
            tables.append(kernel_table(code_objects_of(lib, d)))
        old, new = tables
        for tag, lib, table in (("old", args.old, old), ("new", args.new, new)):
            print(f"{tag}: {lib}  " + (f"build id {build_id(lib)}  " if lib.endswith(".so") else "") + f"{len(table)} kernels")
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
