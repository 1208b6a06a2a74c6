"""What compiling an SDF program buys (profiles/program_compile.json is this tool's output).

    python tools/program_compile_bench.py [--launches 24] > profiles/program_compile.json

For `demo3` (3 instructions), `spheres8` (39) and `example_sixteen` (77), in ONE process, the interpreted handle and the handle
sdfv_program_compile made of it alternated launch by launch after a warm-up, device events around every launch, medians:
  fill    the fused fill at 256^3 with the plain distance volume (36 B/voxel),
  points  sdfv_program_sample_points over 2^24 points,
  march   sdfv_program_raymarch at 1920 x 1080 from eye (1.9, 2.3, 3.8),
and compile_seconds / code_bytes per route.  The yardstick is the interpreted handle of the same run (today's kernels:
profiles/kernel_diff_program_compile.txt).  Stamped with sdfv_build_id() and the box."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    import source_hash
    from program_mesh_bench import spheres8

    builders = {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract(), "spheres8": spheres8(PM), "example_sixteen": PM.example_sixteen()}
    side, n_points, width, height = 256, 1 << 24, 1920, 1080
    g = pkg.make_grid((side, side, side))
    t0, t1 = pkg.alloc_textures(g)
    dist = torch.empty((side, side, side), device="cuda")
    pts = (torch.rand((n_points, 3), device="cuda") * 2.4 - 1.2).contiguous()
    rec = torch.empty((n_points, 7), device="cuda")
    rgba = torch.empty((1, height, width, 4), device="cuda")
    cam = pkg.camera_look_at(eye=(1.9, 2.3, 3.8), aspect=width / height)
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "launches": args.launches, "warmup": args.warmup, "fill_side": side, "points": n_points, "march": [width, height], "programs": {}}
    for name, b in builders.items():
        plain = b.build()
        res = {"ops": len(b.ops)}
        routes = {"fill": (PM.FILL, lambda p: p.fill_grid(g, t0, t1, dist=dist)),
                  "points": (PM.POINTS, lambda p: p.sample_points(pts, out=rec)),
                  "march": (PM.MARCH, lambda p: p.render(cam, width, height, out=rgba))}
        for route, (bit, call) in routes.items():
            comp = plain.compile(bit)
            info = comp.compiled_info()
            handles = {"interpreted": plain, "compiled": comp}
            for _ in range(args.warmup):
                for p in handles.values():
                    call(p)
            torch.cuda.synchronize()
            ms = {k: [] for k in handles}
            for _ in range(args.launches):
                for k, p in handles.items():          # alternated: both see the same drift of clocks and neighbours
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(p)
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            med = {k: statistics.median(v) for k, v in ms.items()}
            res[route] = {"interpreted_ms_median": round(med["interpreted"], 5), "compiled_ms_median": round(med["compiled"], 5),
                          "interpreted_ms_min": round(min(ms["interpreted"]), 5), "compiled_ms_min": round(min(ms["compiled"]), 5),
                          "interpreted_over_compiled": round(med["interpreted"] / med["compiled"], 3),
                          "compile_seconds": round(info["compile_seconds"], 3), "code_bytes": info["code_bytes"],
                          "specialised_launches": comp.compiled_info()["launches"]}
            comp.close()
        out["programs"][name] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
