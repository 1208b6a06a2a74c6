"""What sparse meshing of an SDF program costs against the dense extractor of the same build (profiles/sparse_mesh.json is this
tool's output).

    python tools/sparse_mesh_bench.py --timing TIMING.json                        # the times: profiler off
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/sparse_mesh_bench.py --cells 1024 --sparse-only "" --rounds 5 --timing TRACE/timing.json
    python tools/sparse_mesh_bench.py --merge TIMING.json --from-trace TRACE --trace-timing TRACE/timing.json > profiles/sparse_mesh.json

Marching cubes with SDFV_MESH_WITH_MATERIALS of example_sixteen (77 instructions; no surface in its box, so the vertex phase is
empty and the refinement and the brick lattice are all there is) and spheres8 (tools/program_mesh_bench.py's eight blended
spheres), in ONE process after a warm-up of every shape:
  256 and 1024 cells   sdfv_program_mesh_extract and sdfv_program_mesh_extract_sparse, alternated call by call;
  2048 and 4096 cells  sparse alone (the dense extractor stops at 1024), with the scratch it needed.
A call is timed by a host clock around the C call, which ends in a synchronise of its stream; the mesh is freed outside the
timed span.  The yardsticks are the dense route in the same run and the evaluation ratio from the stats: (cells + 1)^3 program
runs of the dense lattice over `evaluations` of the sparse call -- both before the vertex phase, which the two routes share.
The kernel trace is a run of its own (tracing changes the host side of a call): it gives the device time of the refinement
(sdfprog_sparse_refine, its scans, sparse_compact), of the brick lattice (sdfprog_sparse_bricks) and of the rest, and what is left
of a call's span between its first and last kernel -- the gaps the per-level host reads leave.
Stamped with sdfv_build_id()."""
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


def cells_of(text):
    return [int(c) for c in text.split(",") if c]


def run(args):
    import torch
    from program_mesh_bench import spheres8
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    K, lib = pkg._capi, pkg.lib
    progs = {"example_sixteen": PM.example_sixteen().build(), "spheres8": spheres8(PM).build()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dense(p, n):
        m = K.Mesh()
        t0 = time.perf_counter()
        rc = lib.sdfv_program_mesh_extract(p.h, None, None, n, 0, K.MESH_WITH_MATERIALS, C.byref(m), stream)
        ms = (time.perf_counter() - t0) * 1e3
        pkg.check(rc)
        out = dict(ms=ms, vertices=int(m.n_vertices), triangles=int(m.n_indices) // 3)
        lib.sdfv_mesh_free(C.byref(m))
        return out

    def sparse(p, n):
        m, s, d = K.Mesh(), K.SparseMeshStats(), K.SparseMeshDesc()
        s.size, d.size = C.sizeof(s), C.sizeof(d)
        d.program, d.cells, d.flags, d.out, d.stats = p.h, n, K.MESH_WITH_MATERIALS, C.pointer(m), C.pointer(s)
        t0 = time.perf_counter()
        rc = lib.sdfv_program_mesh_extract_sparse(C.byref(d), stream)
        ms = (time.perf_counter() - t0) * 1e3
        pkg.check(rc)
        out = dict(ms=ms, vertices=int(m.n_vertices), triangles=int(m.n_indices) // 3,
                   stats=dict(levels=s.levels, tested=list(s.tested[:s.levels]), kept=list(s.kept[:s.levels]), bricks=s.bricks,
                              evaluations=s.evaluations, scratch_bytes=s.scratch_bytes))
        lib.sdfv_mesh_free(C.byref(m))
        return out

    both, alone = cells_of(args.cells), cells_of(args.sparse_only)
    seq, calls = [], {}
    for n in both + alone:
        variants = [(k, r) for k in progs for r in (("dense", "sparse") if n in both else ("sparse",))]
        for phase, count in (("warmup", args.warmup), ("timed", args.rounds)):
            for _ in range(count):
                for k, route in variants:                       # alternated: every variant sees the same drift
                    r = (dense if route == "dense" else sparse)(progs[k], n)
                    seq.append([k, route, n, phase])
                    if phase == "timed":
                        c = calls.setdefault(f"{k}/{route}@{n}", dict(ms=[]))
                        c["ms"].append(r.pop("ms"))
                        c.update(r)
    out_calls = {}
    for key, c in calls.items():
        ms = c.pop("ms")
        out_calls[key] = dict(ms_median=statistics.median(ms), ms_min=min(ms), **c)
    ratios = {}
    for n in both:
        for k in progs:
            d, s = out_calls[f"{k}/dense@{n}"], out_calls[f"{k}/sparse@{n}"]
            assert (d["vertices"], d["triangles"]) == (s["vertices"], s["triangles"]), (k, n, d, s)
            evals = (n + 1) ** 3 / s["stats"]["evaluations"]
            speed = d["ms_median"] / s["ms_median"]
            ratios[f"{k}@{n}"] = dict(dense_over_sparse_ms=round(speed, 3), dense_over_sparse_evaluations=round(evals, 3),
                                      time_ratio_over_evaluation_ratio=round(speed / evals, 3))
    lib.sdfv_mesh_trim()
    out = dict(build_id=lib.sdfv_build_id().decode(), device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup,
               sequence=seq, calls=out_calls, ratios=ratios,
               method="calls: a host clock around each C call (it ends in a stream synchronise), one process, profiler off, dense and "
                      "sparse alternated after a warm-up of every shape; the mesh is freed outside the timed span")
    os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
    json.dump(out, open(args.timing, "w"), indent=1)
    print("wrote", args.timing)
    print(json.dumps(dict(calls={k: round(v["ms_median"], 3) for k, v in out_calls.items()}, ratios=ratios), indent=1))


def phase_of(name, state):
    """(phase, next state) of a kernel by its name and by where its extraction stands: the rocPRIM scans serve both routes and, in
    the sparse one, both the refinement and the counting."""
    if "sdfprog_sparse_refine" in name:
        return "refinement", "refine"
    if "sdfprog_sparse_bricks" in name:
        return "brick_lattice", "bricks"
    if "sdfprog_mesh_lattice" in name:
        return None, "dense"
    if state == "refine" and ("sparse_compact" in name or "rocprim" in name or "scan" in name):
        return "refinement", state
    if state == "bricks":
        if "sdfprog_mesh_vertices" in name:
            return "vertices", state
        if "sparse_brick_" in name or "rocprim" in name or "scan" in name:
            return "count_positions_triangles", state
    return None, state


def from_trace(args):
    timing = json.load(open(args.trace_timing))
    rows = []
    for f in glob.glob(os.path.join(args.from_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    groups, state = [], None
    for start, end, name in rows:
        was = state
        phase, state = phase_of(name, state)
        if phase == "refinement" and was != "refine":
            groups.append(dict(first=start, last=end, phases={}))
        if phase and groups:
            g = groups[-1]
            g["phases"][phase] = g["phases"].get(phase, 0) + (end - start)
            g["last"] = max(g["last"], end)
    sparse_seq = [s for s in timing["sequence"] if s[1] == "sparse"]
    assert len(groups) == len(sparse_seq), (len(groups), len(sparse_seq))
    acc = {}
    for (k, _, n, kind), g in zip(sparse_seq, groups):
        if kind == "timed":
            acc.setdefault(f"{k}/sparse@{n}", []).append(g)
    names = ("refinement", "brick_lattice", "count_positions_triangles", "vertices")
    trace = {}
    for key, gs in acc.items():
        t = {p: round(statistics.median([g["phases"].get(p, 0) for g in gs]) / 1e3, 2) for p in names}          # microseconds
        t["kernels_sum_us"] = round(sum(t[p] for p in names), 2)
        t["first_to_last_kernel_us"] = round(statistics.median([g["last"] - g["first"] for g in gs]) / 1e3, 2)
        t["gaps_us"] = round(t["first_to_last_kernel_us"] - t["kernels_sum_us"], 2)
        t["call_ms_median_under_the_tracer"] = round(timing["calls"][key]["ms_median"], 3)
        trace[key] = t
    out = json.load(open(args.merge))
    out.pop("sequence", None)
    out["kernel_trace"] = dict(build_id=timing["build_id"], rounds=timing["rounds"], phases_us_median=trace,
                               method="kernel durations (device timestamps) of a rocprofv3 --kernel-trace --stats run of its own; gaps = "
                                      "first kernel's start to last kernel's end, less the kernels' durations")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="256,1024", help="both routes")
    ap.add_argument("--sparse-only", default="2048,4096")
    ap.add_argument("--timing", default="sparse_mesh_timing.json")
    ap.add_argument("--merge", default="", help="the timing file of the untraced run")
    ap.add_argument("--from-trace", default="")
    ap.add_argument("--trace-timing", default="")
    a = ap.parse_args()
    from_trace(a) if a.from_trace else run(a)
