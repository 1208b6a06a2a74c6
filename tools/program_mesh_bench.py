"""What meshing an SDF program costs, phase by phase (profiles/program_mesh.json is this tool's output).

    rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/program_mesh_bench.py --rounds 12 --timing TRACE/timing.json
    python tools/program_mesh_bench.py --from-trace TRACE --timing TRACE/timing.json > profiles/program_mesh.json

Marching cubes at 128 and 256 cells of
  demo             the demo tree through sdfv_mesh_extract,
  demo3            CUBE 0.95, SPHERE 1.05, SUBTRACT: the demo's distance as a program,
  spheres8         eight blended spheres (39 instructions),
  example_sixteen  the 16-primitive model (77 instructions; no surface in its box: the lattice phase alone),
through sdfv_program_mesh_extract with SDFV_MESH_WITH_MATERIALS, alternated variant by variant in ONE process after a warm-up.
An extraction synchronises in the middle (the output size is data dependent), so its phases cannot be bracketed by events from
outside the library: the per-phase times are the DEVICE timestamps of the kernels in a rocprofv3 kernel trace of that same
process (a run of its own: tracing is not combined with counters), grouped by kernel name --
  lattice    lattice_kernel / sdfprog_mesh_lattice
  count      edge_mask_kernel, cell_count_kernel, the rocPRIM scan kernels, totals_kernel
  positions  mesh_edge_positions                          (the demo writes positions in its fused vertex kernel)
  vertices   emit_vertices_kernel / sdfprog_mesh_vertices[_mat]
  triangles  emit_triangles_kernel
-- median over the rounds, per (variant, cells); a variant's kernels are told apart by the order of the process's dispatches,
which this run records (timing.json: the sequence of (variant, cells) and the whole-call event times).  In the same process the
dense fill of each program at 256^3 gives the interpreter's voxels/s for the lattice phase to be read against.
Ratios recorded, none of them a threshold: program / demo for demo3; lattice points/s over fill voxels/s; vertices / lattice.
Stamped with sdfv_build_id()."""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = (("lattice", ("lattice_kernel", "sdfprog_mesh_lattice")),
          ("count", ("edge_mask_kernel", "cell_count_kernel", "totals_kernel", "rocprim", "scan")),
          ("positions", ("mesh_edge_positions",)),
          ("vertices", ("emit_vertices_kernel", "sdfprog_mesh_vertices")),
          ("triangles", ("emit_triangles_kernel",)))


def phase_of(kernel):
    for phase, keys in PHASES:
        if any(k in kernel for k in keys):
            return phase
    return None


def spheres8(PM):
    import math
    s = PM.Program()
    for i in range(8):
        ang = math.radians(45.0 * i)
        s.material(0.1 + 0.1 * i, 0.9 - 0.1 * i, 0.5, 0.1 * i, 0.5, 1.0)
        s.push_affine(PM.translation(0.55 * math.cos(ang), 0.55 * math.sin(ang), 0.1 * (i % 3 - 1))).sphere(0.22).pop()
        if i:
            s.smooth_union(0.1)
    return s


def run(args):
    import torch
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    prm = pkg.default_params()
    builders = {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract(), "spheres8": spheres8(PM),
                "example_sixteen": PM.example_sixteen()}
    progs = {k: b.build() for k, b in builders.items()}
    variants = {"demo": lambda n: pkg.mesh_extract(prm, n)}
    for k, p in progs.items():
        variants[k] = (lambda n, p=p: p.mesh(n, materials=True))
    seq, calls = [], {}
    cells = [int(c) for c in args.cells.split(",")]
    for n in cells:
        for _ in range(args.warmup):
            for k, fn in variants.items():
                fn(n)
                seq.append([k, n, "warmup"])
        for _ in range(args.rounds):
            for k, fn in variants.items():                 # alternated: every variant sees the same drift
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                v, i = fn(n)
                e1.record()
                e1.synchronize()
                calls.setdefault(f"{k}@{n}", {"ms": [], "vertices": int(v.shape[0]), "triangles": int(i.shape[0]) // 3})["ms"].append(
                    e0.elapsed_time(e1))
                seq.append([k, n, "timed"])
    # the interpreter's rate in the dense fill, same process
    side = 256
    g = pkg.make_grid((side, side, side))
    t0, t1 = pkg.alloc_textures(g)
    dist = torch.empty((side, side, side), device="cuda")
    fill = {}
    for k, p in progs.items():
        ms = []
        for r in range(args.warmup + args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            p.fill_grid(g, t0, t1, dist=dist)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        fill[k] = {"ms_median": statistics.median(ms), "mvoxels_per_s": side ** 3 / statistics.median(ms) / 1e3}
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "warmup": args.warmup, "ops": {k: len(b.ops) for k, b in builders.items()}, "sequence": seq,
           "calls": {k: {"ms_median": statistics.median(c["ms"]), "ms_min": min(c["ms"]), "vertices": c["vertices"],
                         "triangles": c["triangles"]} for k, c in calls.items()},
           "fill_256": fill}
    os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
    json.dump(out, open(args.timing, "w"))
    print("wrote", args.timing)


def from_trace(args):
    timing = json.load(open(args.timing))
    rows = []
    for f in glob.glob(os.path.join(args.from_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    # an extraction = one lattice dispatch and what follows it up to the next one's; they come in the recorded sequence
    groups = []
    for start, end, name in rows:
        phase = phase_of(name)
        if phase == "lattice":
            groups.append({})
        if phase and groups:
            groups[-1][phase] = groups[-1].get(phase, 0) + (end - start)
    mesh_seq = timing["sequence"]
    assert len(groups) >= len(mesh_seq), (len(groups), len(mesh_seq))
    groups = groups[:len(mesh_seq)]          # (the fill's kernels that follow hold no lattice dispatch)
    acc = {}
    for (variant, n, kind), g in zip(mesh_seq, groups):
        if kind == "timed":
            acc.setdefault(f"{variant}@{n}", []).append(g)
    phases = {}
    for key, gs in acc.items():
        phases[key] = {p: round(statistics.median([g.get(p, 0) for g in gs]) / 1e3, 2) for p, _ in PHASES}   # microseconds
        phases[key]["sum_us"] = round(sum(phases[key].values()), 2)
    ratios = {}
    for key, ph in phases.items():
        variant, n = key.split("@")
        n = int(n)
        r = {}
        if variant != "demo":
            points = (n + 1) ** 3
            r["lattice_mpoints_per_s"] = round(points / ph["lattice"], 1)
            r["lattice_points_per_s_over_fill_voxels_per_s"] = round(points / ph["lattice"] / timing["fill_256"][variant]["mvoxels_per_s"], 3)
            if ph["lattice"]:
                r["vertices_over_lattice"] = round(ph["vertices"] / ph["lattice"], 3)
        if variant == "demo3":
            r["program_over_demo_sum"] = round(ph["sum_us"] / phases[f"demo@{n}"]["sum_us"], 3)
        ratios[key] = r
    out = {k: timing[k] for k in ("build_id", "device", "rounds", "warmup", "ops", "calls", "fill_256")}
    out["phases_us_median"] = phases
    out["ratios"] = ratios
    out["method"] = "phases: kernel durations (device timestamps) of a rocprofv3 --kernel-trace run of the timed process; calls: device events around whole extractions in that run"
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="128,256")
    ap.add_argument("--timing", default="program_mesh_timing.json")
    ap.add_argument("--from-trace", default="")
    a = ap.parse_args()
    from_trace(a) if a.from_trace else run(a)
