"""What compiling an SDF program buys its mesh route, SDFV_COMPILE_MESH (profiles/program_compile_mesh.json is this tool's
output).

    python tools/program_compile_mesh_bench.py --timing TIMING.json                    # the times: profiler off
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_PLAIN -- python tools/program_compile_mesh_bench.py --trace plain --timing TRACE_PLAIN/sections.json
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_COMPILED -- python tools/program_compile_mesh_bench.py --trace compiled --timing TRACE_COMPILED/sections.json
    python tools/program_compile_mesh_bench.py --merge TIMING.json --from-trace TRACE_PLAIN TRACE_COMPILED > profiles/program_compile_mesh.json

For `demo3` (3 instructions), `spheres8` (39) and `example_sixteen` (77), in ONE process, the plain handle and the handle
compiled with MESH alternated call by call after a warm-up of every shape, a host clock around each C call (the extractors end
in a synchronise of their stream; the two point-list calls are followed by one inside the timed span), medians of 9:
  mc256        sdfv_program_mesh_extract, marching cubes at 256 cells with SDFV_MESH_WITH_MATERIALS,
  dc256        ... dual contouring at 256 cells,
  sparse256, sparse1024   sdfv_program_mesh_extract_sparse with materials,
  normals      sdfv_program_normal_points over 2^24 points,
and compile_seconds / code_bytes of the route.  The yardstick is the plain handle of the same run; `spread` is the plain
handle's own max - min over its nine repeats.  The per-kernel times come from two runs of their own under the kernel tracer, one
per handle kind, in which nothing else is traced (they add normal_points over 2^20 points off a 16-byte boundary and
mesh_postproc over 2^20 - 1 vertices, aligned and not, so that all nine kernels run): every (program, row) is one section of
--trace-rounds calls, the sections parted by one launch of the SDF-free lattice_points kernel (a program's warm-up is a
section of its own, dropped), and a kernel's time is the sum of its durations in the section over the calls.  Stamped with
sdfv_build_id() and the box."""
import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROWS = ("mc256", "dc256", "sparse256", "sparse1024", "normals")
KERNELS = ("mesh_lattice", "mesh_vertices", "mesh_vertices_mat", "normal_points", "normal_points_staged", "mesh_postproc",
           "mesh_postproc_unaligned", "sparse_refine", "sparse_bricks")


def setup():
    import torch
    from program_mesh_bench import spheres8
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    K, lib = pkg._capi, pkg.lib
    builders = {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract(), "spheres8": spheres8(PM), "example_sixteen": PM.example_sixteen()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_points = 1 << 24
    pts = (torch.rand((n_points, 3), device="cuda") * 2.4 - 1.2).contiguous()
    normals = torch.empty((n_points, 3), device="cuda")
    verts = torch.zeros((1 << 20, 12), device="cuda")      # (the tracer's postproc sections: positions, normals unset)
    verts[:, :3] = pts[:1 << 20]

    def dense(p, n, algorithm):
        m = K.Mesh()
        t0 = time.perf_counter()
        rc = lib.sdfv_program_mesh_extract(p.h, None, None, n, algorithm, K.MESH_WITH_MATERIALS, C.byref(m), stream)
        ms = (time.perf_counter() - t0) * 1e3
        pkg.check(rc)
        out = dict(ms=ms, vertices=int(m.n_vertices), indices=int(m.n_indices))
        lib.sdfv_mesh_free(C.byref(m))
        return out

    def sparse(p, n):
        m, d = K.Mesh(), K.SparseMeshDesc()
        d.size = C.sizeof(d)
        d.program, d.cells, d.flags, d.out = p.h, n, K.MESH_WITH_MATERIALS, C.pointer(m)
        t0 = time.perf_counter()
        rc = lib.sdfv_program_mesh_extract_sparse(C.byref(d), stream)
        ms = (time.perf_counter() - t0) * 1e3
        pkg.check(rc)
        out = dict(ms=ms, vertices=int(m.n_vertices), indices=int(m.n_indices))
        lib.sdfv_mesh_free(C.byref(m))
        return out

    def point_normals(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.normal_points(pts, 0.0, out=normals)
        torch.cuda.synchronize()
        return dict(ms=(time.perf_counter() - t0) * 1e3)

    def point_normals_unaligned(p):                        # (the tracer's: arrays off a 16-byte boundary, all n through the tail kernel)
        n = 1 << 20
        p.normal_points(pts.view(-1)[1:1 + 3 * n].view(n, 3), 0.0, out=normals.view(-1)[1:1 + 3 * n].view(n, 3))
        torch.cuda.synchronize()
        return dict(ms=0.0)

    def postproc(p, off):
        v = verts.view(-1)[off:off + ((1 << 20) - 1) * 12].view(-1, 12)
        v.zero_()                                          # normals unset: every vertex takes the taps
        v[:, :3] = pts[:v.shape[0]]
        p.mesh_postproc(v)
        torch.cuda.synchronize()
        return dict(ms=0.0)

    calls = {"mc256": lambda p: dense(p, 256, K.MESHER_MARCHING_CUBES), "dc256": lambda p: dense(p, 256, K.MESHER_DUAL_CONTOURING_PARTICLE),
             "sparse256": lambda p: sparse(p, 256), "sparse1024": lambda p: sparse(p, 1024), "normals": point_normals, "normals_unaligned": point_normals_unaligned,
             "postproc": lambda p: postproc(p, 0), "postproc_unaligned": lambda p: postproc(p, 1)}
    return torch, pkg, PM, builders, calls


def run(args):
    import source_hash
    torch, pkg, PM, builders, calls = setup()
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "warmup": args.warmup, "programs": {},
           "method": "a host clock around each C call (the extractors end in a stream synchronise; normal_points is followed by one "
                     "inside the span), one process, profiler off, the plain and the compiled handle alternated after a warm-up of "
                     "every shape; spread = the plain handle's max - min over its repeats"}
    for name, b in builders.items():
        plain = b.build()
        comp = plain.compile(PM.MESH)
        info = comp.compiled_info()
        handles = {"plain": plain, "compiled": comp}
        res = {"ops": len(b.ops), "compile_seconds": round(info["compile_seconds"], 3), "code_bytes": info["code_bytes"]}
        for row in ROWS:
            for _ in range(args.warmup):
                for p in handles.values():
                    calls[row](p)
        for row in ROWS:
            ms = {k: [] for k in handles}
            shape = {}
            for _ in range(args.rounds):
                for k, p in handles.items():          # alternated: both see the same drift of clocks and neighbours
                    r = calls[row](p)
                    ms[k].append(r.pop("ms"))
                    assert shape.setdefault("mesh", r) == r, (name, row, shape, r)   # both handles, every round: the same counts
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = max(ms["plain"]) - min(ms["plain"])
            res[row] = {"plain_ms_median": round(med["plain"], 4), "compiled_ms_median": round(med["compiled"], 4),
                        "plain_ms_min": round(min(ms["plain"]), 4), "compiled_ms_min": round(min(ms["compiled"]), 4),
                        "plain_spread_ms": round(spread, 4), "plain_over_compiled": round(med["plain"] / med["compiled"], 3),
                        "compiled_within_plain_spread": bool(med["compiled"] <= med["plain"] + spread), **shape.get("mesh", {})}
        res["specialised_launches"] = comp.compiled_info()["launches"]
        assert plain.compiled_info()["launches"] == 0
        out["programs"][name] = res
        comp.close()
    pkg.lib.sdfv_mesh_trim()
    os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
    json.dump(out, open(args.timing, "w"), indent=1)
    print("wrote", args.timing)
    print(json.dumps({n: {r: (v[r]["plain_ms_median"], v[r]["compiled_ms_median"]) for r in ROWS} for n, v in out["programs"].items()}, indent=1))


def trace(args):
    """One handle kind, nothing but kernels traced: sections of args.trace_rounds calls, each begun by one lattice_points launch."""
    torch, pkg, PM, builders, calls = setup()
    sections = []
    rows = ROWS + ("normals_unaligned", "postproc", "postproc_unaligned")
    for name, b in builders.items():
        p = b.build()
        if args.trace == "compiled":
            p = p.compile(PM.MESH)
        pkg.lattice_points((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), 1)
        for row in rows:
            calls[row](p)                                  # warm: scratch, clocks -- a section of its own, dropped by --merge
        sections.append([name, "warmup", 1])
        for row in rows:
            pkg.lattice_points((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), 1)
            for _ in range(args.trace_rounds):
                calls[row](p)
            sections.append([name, row, args.trace_rounds])
        assert (p.compiled_info()["launches"] > 0) == (args.trace == "compiled")
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
    json.dump({"kind": args.trace, "build_id": pkg.lib.sdfv_build_id().decode(), "sections": sections}, open(args.timing, "w"), indent=1)
    print("wrote", args.timing)


def kernel_of(name):
    """"mesh_lattice" for sdfprog_mesh_lattice(...) and sdfprogc_mesh_lattice(...), None for any other kernel."""
    base = name.split("(")[0].strip()
    for prefix in ("sdfprogc_", "sdfprog_"):
        if base.startswith(prefix) and base[len(prefix):] in KERNELS:
            return base[len(prefix):]
    return None


def section_times(directory):
    """{program: {row: {kernel: microseconds per call}}} of one traced run."""
    found = glob.glob(os.path.join(directory, "**", "sections.json"), recursive=True)
    assert len(found) == 1, found
    meta = json.load(open(found[0]))
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    per_section, current = [], None
    for start, end, name in rows:
        if "lattice_points" in name and "sdfprog" not in name:
            current = {}
            per_section.append(current)
        elif current is not None and kernel_of(name):
            current[kernel_of(name)] = current.get(kernel_of(name), 0) + (end - start)
    assert len(per_section) == len(meta["sections"]), (len(per_section), len(meta["sections"]))
    out = {}
    for (prog, row, calls), t in zip(meta["sections"], per_section):
        if row != "warmup":
            out.setdefault(prog, {})[row] ={k: round(v / calls / 1e3, 2) for k, v in sorted(t.items())}
    return meta, out


def merge(args):
    out = json.load(open(args.merge))
    (meta_p, plain), (meta_c, comp) = section_times(args.from_trace[0]), section_times(args.from_trace[1])
    assert meta_p["kind"] == "plain" and meta_c["kind"] == "compiled"
    table, verdict = {}, {}
    for prog in plain:
        for row in plain[prog]:
            for k, us in plain[prog][row].items():
                c = comp[prog][row].get(k)
                table.setdefault(prog, {}).setdefault(row, {})[k] = {"plain_us": us, "compiled_us": c,
                                                                     "plain_over_compiled": round(us / c, 3) if c else None}
                if c is not None:
                    v = verdict.setdefault(k, {}).setdefault(prog, True)
                    verdict[k][prog] = v and c < us
    out["kernel_trace"] = {"build_id": meta_p["build_id"], "per_call_us": table, "compiled_below_plain_in_every_section": verdict,
                           "method": "kernel durations (device timestamps) of two rocprofv3 --kernel-trace --stats runs of their own, one "
                                     "per handle kind; per section the sum of a kernel's durations over the section's calls"}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timing", default="program_compile_mesh_timing.json")
    ap.add_argument("--trace", choices=["plain", "compiled"], default=None, help="the run under the kernel tracer, one handle kind")
    ap.add_argument("--trace-rounds", type=int, default=3)
    ap.add_argument("--merge", default="", help="the timing file of the untraced run")
    ap.add_argument("--from-trace", nargs=2, default=None, metavar=("PLAIN_DIR", "COMPILED_DIR"))
    a = ap.parse_args()
    if a.from_trace:
        merge(a)
    elif a.trace:
        trace(a)
    else:
        run(a)
