"""What an SDF program costs against the demo's fill (profiles/program_fill.json is this tool's output).

    python tools/program_bench.py [--launches 24] [--sides 256,512] [--no-load] > profiles/program_fill.json

Fused fill (textures + plain distance volume, 36 B/voxel) of
  A  the demo through sdfv_fill_grid_commit (the kernel every earlier profile times),
  B  the program CUBE 0.95, SPHERE 1.05, SUBTRACT (the demo's distance as a program),
  C  a 16-primitive program with frames and materials (sdf-viewer_amd/program.py: example_sixteen),
alternated A B C A B C ... in ONE process after a warm-up, device events around every launch, the median and the minimum per
variant; Mvoxels/s and the fraction of an 8 TB/s roofline on 36 B/voxel; B / A and C / A.  Then, at 256^3,
  D  a full 3-pass load of program C through the viewer's device route (sdfv_program_as_surface),
  E  the same surface with the device sampler cleared: the host route on up to 16 threads,
wall-clock per load (the viewer's calls synchronise), D / E, and C against D.
Stamped with sdfv_build_id() and the box."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROOFLINE_BYTES_PER_S = 8.0e12
BYTES_PER_VOXEL = 36


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sides", default="256,512")
    ap.add_argument("--no-load", action="store_true", help="skip the viewer loads D and E")
    ap.add_argument("--only", default="", help="run ONE variant (A, B or C) at the first side, for a kernel trace")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    import source_hash

    prm = pkg.default_params()
    prog_b = PM.Program().cube(0.95).sphere(1.05).subtract().build()
    builder_c = PM.example_sixteen()
    prog_c = builder_c.build()
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "launches": args.launches, "warmup": args.warmup, "bytes_per_voxel": BYTES_PER_VOXEL,
           "roofline_TBps": ROOFLINE_BYTES_PER_S / 1e12, "ops": {"B": 3, "C": len(builder_c.ops)}, "fill": {}}
    for side in [int(s) for s in args.sides.split(",")]:
        g = pkg.make_grid((side, side, side))
        t0, t1 = pkg.alloc_textures(g)
        dist = torch.empty((side, side, side), device="cuda")
        variants = {"A": lambda: pkg.fill_grid(prm, g, t0, t1, dist=dist),
                    "B": lambda: prog_b.fill_grid(g, t0, t1, dist=dist),
                    "C": lambda: prog_c.fill_grid(g, t0, t1, dist=dist)}
        if args.only:
            variants = {args.only: variants[args.only]}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.launches):
            for k, fn in variants.items():          # alternated: every variant sees the same drift of clocks and neighbours
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        res = {}
        n = side ** 3
        for k, v in ms.items():
            med = statistics.median(v)
            res[k] = {"ms_median": round(med, 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5),
                      "mvoxels_per_s": round(n / med / 1e3, 1),
                      "roofline_fraction": round(n * BYTES_PER_VOXEL / (med * 1e-3) / ROOFLINE_BYTES_PER_S, 4)}
        if "A" in res:
            for k in list(res):
                if k != "A":
                    res[k + "_over_A_rate"] = round(res["A"]["ms_median"] / res[k]["ms_median"], 4)
        out["fill"][str(side)] = res
        del t0, t1, dist
        torch.cuda.empty_cache()
        if args.only:
            break
    if not args.no_load and not args.only:
        V = importlib.import_module("sdf-viewer_amd.viewer")
        side = 256
        loads = {}
        for route in ("D_device_route", "E_host_route"):
            surf = prog_c.as_surface(device_route=route.startswith("D"))
            times = []
            for _ in range(3):
                v = V.Viewer.new_voxels((side, side, side), builder_c.bb, 3)
                if route.startswith("E"):
                    v.set_ingest(host_threads=16)
                torch.cuda.synchronize()
                t = time.perf_counter()
                while v.state()["remaining"]:
                    v.update(surf, budget_s=10.0)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t)
                v.close()
            visited = side ** 3 + (side // 2) ** 3 + (side // 4) ** 3
            best = min(times)
            loads[route] = {"seconds": [round(x, 5) for x in times], "seconds_min": round(best, 5),
                            "mvoxels_per_s_of_the_grid": round(side ** 3 / best / 1e6, 1), "samples_taken": visited}
        loads["D_over_E_rate"] = round(loads["E_host_route"]["seconds_min"] / loads["D_device_route"]["seconds_min"], 2)
        if "256" in out["fill"] and "C" in out["fill"]["256"]:
            loads["dense_C_over_D_rate"] = round(loads["D_device_route"]["seconds_min"] * 1e3 / out["fill"]["256"]["C"]["ms_median"], 2)
        out["load_256"] = loads
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
