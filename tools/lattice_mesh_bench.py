"""What meshing a sampled lattice costs against meshing the program the lattice came from (profiles/lattice_mesh.json is this
tool's output).

    rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/lattice_mesh_bench.py --rounds 12 --timing TRACE/timing.json
    python tools/lattice_mesh_bench.py --from-trace TRACE --timing TRACE/timing.json > profiles/lattice_mesh.json

Marching cubes at 128 and 256 cells of demo3 (CUBE 0.95, SPHERE 1.05, SUBTRACT) and spheres8 (tools/program_mesh_bench.py's),
each through sdfv_program_mesh_extract and through sdfv_lattice_mesh_extract over that program's own distances at the lattice
points (sdfv_lattice_points -> the program's point sampler -> sdfv_lattice_from_samples, made once, outside the timed calls),
alternated variant by variant in ONE process after a warm-up.  The program route in the same process is the yardstick: the
lattice route runs the same SDF-free phases, nothing in the place of the interpreter's lattice pass and a gather in the place of
its four-tap vertex phase, so it should not be slower.
Per-phase times are the DEVICE timestamps of the kernels in a rocprofv3 kernel trace of that same process (a run of its own),
grouped by kernel name as tools/program_mesh_bench.py groups them -- an extraction starts at its edge_mask_kernel dispatch, a
lattice dispatch belongs to the extraction that follows it -- and matched to (variant, cells) by the recorded order of the calls.
The host-sampled route of mesh_any_sdf is not timed here: it is bound by the caller's sample().
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

PHASES = (("lattice", ("sdfprog_mesh_lattice",)),
          ("count", ("edge_mask_kernel", "cell_count_kernel", "totals_kernel", "rocprim", "scan")),
          ("positions", ("mesh_edge_positions",)),
          ("vertices", ("sdfprog_mesh_vertices", "lattice_normals")),
          ("triangles", ("emit_triangles_kernel",)))


def phase_of(kernel):
    for phase, keys in PHASES:
        if any(k in kernel for k in keys):
            return phase
    return None


def run(args):
    import torch
    from program_mesh_bench import spheres8
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    bb = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    progs = {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract().build(), "spheres8": spheres8(PM).build()}
    seq, calls = [], {}
    for n in [int(c) for c in args.cells.split(",")]:
        variants = {}
        for k, p in progs.items():
            dist = pkg.lattice_from_samples(p.sample_points(pkg.lattice_points(bb, n), distance_only=True))
            variants[f"{k}/program"] = (lambda p=p: p.mesh(n, bb=bb))
            variants[f"{k}/lattice"] = (lambda dist=dist: pkg.lattice_mesh_extract(dist, bb, n))
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            for k, fn in variants.items():
                fn()
                seq.append([k, n, "warmup"])
        for _ in range(args.rounds):
            for k, fn in variants.items():                 # alternated: every variant sees the same drift
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                v, i = fn()
                e1.record()
                e1.synchronize()
                calls.setdefault(f"{k}@{n}", {"ms": [], "vertices": int(v.shape[0]), "triangles": int(i.shape[0]) // 3})["ms"].append(
                    e0.elapsed_time(e1))
                seq.append([k, n, "timed"])
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "warmup": args.warmup, "sequence": seq,
           "calls": {k: {"ms_median": statistics.median(c["ms"]), "ms_min": min(c["ms"]), "vertices": c["vertices"],
                         "triangles": c["triangles"]} for k, c in calls.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
    json.dump(out, open(args.timing, "w"))
    print("wrote", args.timing)


def from_trace(args):
    timing = json.load(open(args.timing))
    rows = []
    for f in glob.glob(os.path.join(args.from_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    groups, pending = [], 0
    for start, end, name in rows:
        phase = phase_of(name)
        if phase == "lattice":
            pending += end - start
            continue
        if "edge_mask_kernel" in name:
            groups.append({"lattice": pending})
            pending = 0
        if phase and groups:
            groups[-1][phase] = groups[-1].get(phase, 0) + (end - start)
    mesh_seq = timing["sequence"]
    assert len(groups) == len(mesh_seq), (len(groups), len(mesh_seq))
    acc = {}
    for (variant, n, kind), g in zip(mesh_seq, groups):
        assert (g["lattice"] > 0) == variant.endswith("/program"), (variant, n, g)
        if kind == "timed":
            acc.setdefault(f"{variant}@{n}", []).append(g)
    phases = {}
    for key, gs in acc.items():
        phases[key] = {p: round(statistics.median([g.get(p, 0) for g in gs]) / 1e3, 2) for p, _ in PHASES}   # microseconds
        phases[key]["sum_us"] = round(sum(phases[key].values()), 2)
    ratios = {}
    for key, ph in phases.items():
        variant, n = key.split("@")
        if variant.endswith("/lattice"):
            prog = phases[variant[:-len("lattice")] + "program@" + n]
            ratios[key] = {"lattice_over_program_sum": round(ph["sum_us"] / prog["sum_us"], 3),
                           "lattice_over_program_sum_without_its_lattice_phase": round(ph["sum_us"] / (prog["sum_us"] - prog["lattice"]), 3),
                           "gather_over_four_tap_vertices": round(ph["vertices"] / prog["vertices"], 3),
                           "lattice_over_program_call_ms": round(timing["calls"][key]["ms_median"] /
                                                                 timing["calls"][variant[:-len("lattice")] + "program@" + n]["ms_median"], 3)}
    out = {k: timing[k] for k in ("build_id", "device", "rounds", "warmup", "calls")}
    out["phases_us_median"] = phases
    out["ratios"] = ratios
    out["method"] = "phases: kernel durations (device timestamps) of a rocprofv3 --kernel-trace run of the timed process; calls: device events around whole extractions in that run"
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="128,256")
    ap.add_argument("--timing", default="lattice_mesh_timing.json")
    ap.add_argument("--from-trace", default="")
    a = ap.parse_args()
    from_trace(a) if a.from_trace else run(a)
