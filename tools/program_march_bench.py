"""What rendering an SDF program directly costs (profiles/program_march.json is this tool's output).

    python tools/program_march_bench.py [--launches 20] [--host-threads 16] > profiles/program_march.json

One process, device events around every launch, the variants alternated after a warm-up, median and minimum per variant:
  (a) sdfv_program_raymarch at 1080p and 4K of example_sixteen (77 instructions; a frame of misses: its closing plane leaves no
      surface in the box), of the 3-instruction demo program and of eight blended spheres (a model with a surface under every view); the host
      mirror (sdfv_program_raymarch_host) on --host-threads threads for the same frames, wall clock; the speed-up;
  (b) the grid route for context: sdfv_program_fill_grid_commit at 256^3 plus the 1080p grid march over its distance volume;
  (c) evaluations/s = (sum of steps + 5 x hits) / time, next to the dense program fill's voxels/s of the same process, and the
      ratio of the two;
  (d) lane utilisation = sum(steps) / (64 x sum over waves of the wave's max steps), from the steps image, for the kernel's
      8 x 8 tiles and for 64 x 1 rows.
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


def lane_utilisation(steps, tile_w, tile_h):
    import numpy as np
    H, W = steps.shape
    ph, pw = -(-H // tile_h) * tile_h, -(-W // tile_w) * tile_w
    s = np.zeros((ph, pw), np.int64)
    s[:H, :W] = steps
    waves = s.reshape(ph // tile_h, tile_h, pw // tile_w, tile_w).max(axis=(1, 3))
    return float(steps.sum()) / float(64 * waves.sum()) if waves.sum() else 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    import source_hash

    P = PM.Program
    deep = P().material(0.9, 0.9, 0.1, 0.2, 0.4, 1.0)
    for i in range(8):                                   # eight spheres under unions: a model with a surface, 31 instructions
        deep.material(0.1 * i, 1.0 - 0.1 * i, 0.5, 0.1 * i, 0.05 * i, 1.0)
        deep.push_affine(PM.translation(-0.7 + 0.2 * i, 0.5 - 0.14 * i, -0.4 + 0.11 * i)).sphere(0.12 + 0.03 * i).pop()
        if i:
            deep.smooth_union(0.08) if i % 2 else deep.union()
    builders = {"sixteen": PM.example_sixteen(), "demo3": P().cube(0.95).sphere(1.05).subtract(), "spheres8": deep}
    progs = {k: b.build() for k, b in builders.items()}
    g256 = pkg.make_grid((256, 256, 256))
    rp = pkg.default_render_params(g256)
    sizes = {"1080p": (1920, 1080), "4k": (3840, 2160)}
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "launches": args.launches, "warmup": args.warmup, "host_threads": args.host_threads,
           "ops": {k: len(b.ops) for k, b in builders.items()}, "march": {}}

    # the dense fills of this process: (b) and the rate (c) is put next to
    t0, t1 = pkg.alloc_textures(g256)
    dist = torch.empty((256, 256, 256), device="cuda")
    variants = {}
    for name, prog in progs.items():
        variants["fill256_" + name] = (lambda prog=prog: prog.fill_grid(g256, t0, t1, dist=dist))
        for sz, (w, h) in sizes.items():
            cam = pkg.camera_look_at(aspect=w / h, eye=(1.9, 2.3, 3.8))
            variants[f"march_{name}_{sz}"] = (lambda prog=prog, cam=cam, w=w, h=h: prog.render(cam, w, h, rp=rp))
    cam_grid = pkg.camera_look_at(aspect=1920 / 1080, eye=(1.9, 2.3, 3.8))
    progs["spheres8"].fill_grid(g256, t0, t1, dist=dist)
    variants["gridmarch_spheres8_1080p"] = lambda: pkg.raymarch(rp, t0, t1, cam_grid, 1920, 1080, dist=dist)
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.launches):
        for k, fn in variants.items():                  # alternated: every variant sees the same drift of clocks and neighbours
            if k == "gridmarch_spheres8_1080p":
                progs["spheres8"].fill_grid(g256, t0, t1, dist=dist)
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    stat = {k: {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)} for k, v in ms.items()}
    out["fill_256"] = {}
    for name in progs:
        s = stat["fill256_" + name]
        s["mvoxels_per_s"] = round(256 ** 3 / s["ms_median"] / 1e3, 1)
        out["fill_256"][name] = s
    out["grid_route_1080p_spheres8"] = {"fill_256_ms": out["fill_256"]["spheres8"]["ms_median"], "grid_march": stat["gridmarch_spheres8_1080p"],
                                        "fill_plus_march_ms": round(out["fill_256"]["spheres8"]["ms_median"] + stat["gridmarch_spheres8_1080p"]["ms_median"], 5)}
    for name, prog in progs.items():
        for sz, (w, h) in sizes.items():
            cam = pkg.camera_look_at(aspect=w / h, eye=(1.9, 2.3, 3.8))
            _, aux = prog.render(cam, w, h, rp=rp, want_aux=True)
            a = aux[0].cpu().numpy().view(np.int32)
            status, steps = a[..., 0], a[..., 1]
            hits, total = int((status == 1).sum()), int(steps.sum())
            s = dict(stat[f"march_{name}_{sz}"])
            evals = total + 5 * hits
            s.update({"hits": hits, "out_of_bounds": int((status == -2).sum()), "out_of_steps": int((status == -1).sum()),
                      "off_the_box": int((status == 0).sum()), "sum_steps": total, "max_steps": int(steps.max()),
                      "evaluations": evals, "gevaluations_per_s": round(evals / s["ms_median"] / 1e6, 3),
                      "lane_utilisation_8x8": round(lane_utilisation(steps, 8, 8), 4),
                      "lane_utilisation_64x1": round(lane_utilisation(steps, 64, 1), 4)})
            s["evaluation_rate_over_fill_rate"] = round(s["gevaluations_per_s"] * 1e3 / out["fill_256"][name]["mvoxels_per_s"], 4)
            if not args.no_host:
                t = time.perf_counter()
                prog.render_host(cam, w, h, rp=rp, threads=args.host_threads)
                s["host_mirror_s"] = round(time.perf_counter() - t, 4)
                s["device_over_host_speedup"] = round(s["host_mirror_s"] * 1e3 / s["ms_median"], 1)
            out["march"][f"{name}_{sz}"] = s
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
