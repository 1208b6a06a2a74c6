"""What meshing a loaded grid costs against meshing the same distances as a caller's lattice (profiles/grid_mesh.json is this
tool's output).

    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/grid_mesh_bench.py --rounds 12 --timing TRACE/timing.json
    python tools/grid_mesh_bench.py --from-trace TRACE --timing TRACE/timing.json --host-timing TRACE/host.json > profiles/grid_mesh.json
    python tools/grid_mesh_bench.py --host --host-timing TRACE/host.json      (the host comparison, a run of its own, no profiler)

Device.  Marching cubes at 128 and 256 cells of demo3 (CUBE 0.95, SPHERE 1.05, SUBTRACT) and spheres8
(tools/program_mesh_bench.py's), the (cells + 1)^3 grid filled by the program fill, alternated variant by variant in ONE process
after a warm-up:
  lattice      sdfv_lattice_mesh_extract over tex0.r - 0.1f (made once, outside the timed calls): the yardstick, the existing route
               over the same distances in the same process;
  grid/tex0    sdfv_grid_mesh_extract with materials, distances from tex0.r;
  grid/plain   ... from the plain distance volume.
The interleaved layout pairs rows, so it needs an even height, which a cube of cells + 1 voxels with even cells has not: it is
timed on the grid one row higher, (cells + 1) x (cells + 2) x (cells + 1) over a box stretched to keep the voxels cubic, next to
the plain volume of that same grid (grid/plain+row, grid/ilv+row); those two have no lattice yardstick (the lattice route takes
cubes) and are compared with each other.
What the grid route should pay on top of the lattice route is the unpack pass (4 B read + 4 B written per lattice point; 16 B
lines read from tex0) and two 16-byte gathers per vertex.  Per-phase times are the DEVICE timestamps of the kernels in a rocprofv3
kernel trace of that same process, grouped by kernel name -- an extraction starts at its edge_mask_kernel dispatch, an unpack
dispatch belongs to the extraction that follows it -- and matched to (variant, cells) by the recorded order of the calls.

Host, the case that motivates the route.  The gyroid provider (tests/c/gyroid_provider.c, host-only) through
tools/grid_mesh_host_bench.cpp, which this tool builds against the product library: mesh_any_sdf + postproc_any at 128 cells
(sample the 129^3 lattice on the host, mesh, sample every vertex again) against SDFViewer::mesh on a 129^3 grid of the same box
that the viewer has loaded anyway -- the same lattice on both sides, alternated in one process, medians of --host-rounds rounds
after a warm-up round.
Stamped with sdfv_build_id()."""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = (("unpack", ("grid_lattice_",)),
          ("count", ("edge_mask_kernel", "cell_count_kernel", "totals_kernel", "rocprim", "scan")),
          ("positions", ("mesh_edge_positions",)),
          ("vertices", ("lattice_normals", "grid_normals_materials")),
          ("triangles", ("emit_triangles_kernel",)))
INTERLEAVED = 8


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
    seq, calls = [], {}
    for n in [int(c) for c in args.cells.split(",")]:
        variants = {}
        for k in ("demo3", "spheres8"):
            for rows in (n + 1, n + 2):
                top = -1.0 + 2.0 * (rows - 1) / n                              # cubic voxels: the surface is the same one
                bb = (-1.0, -1.0, -1.0, 1.0, top, 1.0)
                b = PM.Program(bb).cube(0.95).sphere(1.05).subtract() if k == "demo3" else spheres8(PM)
                prog = b.build()
                grid = pkg.make_grid((n + 1, rows, n + 1), bb[:3], bb[3:])
                t0, t1 = pkg.alloc_textures(grid)
                dist = torch.empty((n + 1, rows, n + 1), dtype=torch.float32, device="cuda")
                prog.fill_grid(grid, t0, t1, dist=dist)
                if rows == n + 1:
                    lattice = (t0[..., 0] - 0.1).contiguous()
                    variants[f"{k}/lattice"] = (lambda lattice=lattice, bb=bb: pkg.lattice_mesh_extract(lattice, bb, n))
                    variants[f"{k}/grid/tex0"] = (lambda g=grid, t0=t0, t1=t1: pkg.grid_mesh_extract(g, t0, t1, materials=True))
                    variants[f"{k}/grid/plain"] = (lambda g=grid, t0=t0, t1=t1, d=dist: pkg.grid_mesh_extract(g, t0, t1, dist=d, materials=True))
                else:
                    ilv = pkg.commit_interleaved(grid, dist)
                    variants[f"{k}/grid/plain+row"] = (lambda g=grid, t0=t0, t1=t1, d=dist: pkg.grid_mesh_extract(g, t0, t1, dist=d, materials=True))
                    variants[f"{k}/grid/ilv+row"] = (lambda g=grid, t0=t0, t1=t1, d=ilv: pkg.grid_mesh_extract(
                        g, t0, t1, dist=d, volume_flags=INTERLEAVED, materials=True))
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


def host(args):
    """tools/grid_mesh_host_bench.cpp over the gyroid provider: both routes over the same 129^3 lattice, alternated in one process."""
    lib_dir = os.path.join(ROOT, "sdf-viewer_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    tmp = tempfile.mkdtemp(prefix="grid_mesh_bench")
    lib, exe = os.path.join(tmp, "libgyroid_provider.so"), os.path.join(tmp, "grid_mesh_host_bench")
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "gyroid_provider.c"), "-o", lib, "-lm"],
                   check=True, timeout=120)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(lib_dir, "host"), os.path.join(ROOT, "tools", "grid_mesh_host_bench.cpp"), "-o", exe,
                    "-L", lib_dir, "-lsdfviewer_host", "-lsdfgrid", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-Wl,-rpath," + lib_dir, "-ldl", "-pthread"], check=True, timeout=300)
    p = subprocess.run([exe, lib, str(args.host_cells), str(args.host_rounds)], capture_output=True, text=True, check=True,
                       timeout=240)                                           # one GPU process, under a limit of its own
    res = json.loads(p.stdout.strip().split("\n")[-1])
    # the CPUs this process may use: the affinity mask, cut to what the job's environment allows its thread pools
    allowed = [int(os.environ[k]) for k in ("OMP_NUM_THREADS",) if os.environ.get(k, "").isdigit()]
    res.update(provider="tests/c/gyroid_provider.c", cpus=min([len(os.sched_getaffinity(0))] + allowed),
               resample_over_viewer_mesh=round(res["resample_then_mesh_ms"] / res["viewer_mesh_ms"], 2),
               note="both routes over the same lattice: (cells + 1)^3 points of the provider's box; resample = mesh_any_sdf + "
                    "postproc_any, viewer = SDFViewer::mesh with materials on the loaded grid, download included; the viewer's "
                    "load is timed apart")
    json.dump(res, open(args.host_timing, "w"))
    print(json.dumps(res, indent=1))


def from_trace(args):
    timing = json.load(open(args.timing))
    rows = []
    for f in glob.glob(os.path.join(args.from_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    groups, pending = [], 0
    for start, end, name in rows:
        phase = phase_of(name)
        if phase == "unpack":
            pending += end - start
            continue
        if "edge_mask_kernel" in name:
            groups.append({"unpack": pending})
            pending = 0
        if phase and groups:
            groups[-1][phase] = groups[-1].get(phase, 0) + (end - start)
    mesh_seq = timing["sequence"]
    assert len(groups) == len(mesh_seq), (len(groups), len(mesh_seq))
    acc = {}
    for (variant, n, kind), g in zip(mesh_seq, groups):
        assert (g["unpack"] > 0) == ("/grid/" in variant), (variant, n, g)
        if kind == "timed":
            acc.setdefault(f"{variant}@{n}", []).append(g)
    phases = {}
    for key, gs in acc.items():
        phases[key] = {p: round(statistics.median([g.get(p, 0) for g in gs]) / 1e3, 2) for p, _ in PHASES}   # microseconds
        phases[key]["sum_us"] = round(sum(phases[key].values()), 2)
    ratios = {}
    for key, ph in phases.items():
        variant, n = key.split("@")
        model, kind = variant.split("/", 1)
        if kind in ("grid/tex0", "grid/plain"):
            base = phases[f"{model}/lattice@{n}"]
            points, verts = (int(n) + 1) ** 3, timing["calls"][key]["vertices"]
            ratios[key] = {"grid_over_lattice_sum": round(ph["sum_us"] / base["sum_us"], 3),
                           "extra_us": round(ph["sum_us"] - base["sum_us"], 2),
                           "unpack_GBps_of_8B_per_point": round(points * 8 / ph["unpack"] / 1e3, 1) if ph["unpack"] else None,
                           "vertices_over_lattice_vertices": round(ph["vertices"] / base["vertices"], 3),
                           "gather_bytes_per_vertex": 32, "vertices": verts,
                           "grid_over_lattice_call_ms": round(timing["calls"][key]["ms_median"] /
                                                              timing["calls"][f"{model}/lattice@{n}"]["ms_median"], 3)}
        elif kind == "grid/ilv+row":
            base = phases[f"{model}/grid/plain+row@{n}"]
            ratios[key] = {"ilv_over_plain_sum": round(ph["sum_us"] / base["sum_us"], 3),
                           "ilv_over_plain_unpack": round(ph["unpack"] / base["unpack"], 3)}
    out = {k: timing[k] for k in ("build_id", "device", "rounds", "warmup", "calls")}
    out["phases_us_median"] = phases
    out["ratios"] = ratios
    if args.host_timing and os.path.exists(args.host_timing):
        out["host"] = json.load(open(args.host_timing))
    out["method"] = "phases: kernel durations (device timestamps) of a rocprofv3 --kernel-trace run of the timed process; calls: device events around whole extractions in that run; host: the command line's own timers"
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="128,256")
    ap.add_argument("--timing", default="grid_mesh_timing.json")
    ap.add_argument("--host-timing", default="")
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--host-cells", type=int, default=128)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--from-trace", default="")
    a = ap.parse_args()
    host(a) if a.host else (from_trace(a) if a.from_trace else run(a))
