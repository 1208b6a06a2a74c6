"""What casting a list of rays against an SDF program costs (profiles/program_cast.json is this tool's output).

    python tools/program_cast_bench.py [--repeats 9] [--no-host] > profiles/program_cast.json

One process, every shape warmed, medians of --repeats with a host clock around the C call and a device synchronise:
  (a) sdfv_program_raycast over the 1080p primary rays of the march bench's camera (eye (1.9, 2.3, 3.8); 2 073 600 rays built on the
      host by pixel_ray_raw's arithmetic: origin = eye, dir = the raw pixel ray, [0, 1e30]) for demo3, spheres8 and
      example_sixteen, in pixel-row order, in 8 x 8-tile order (64 consecutive rays are one tile) and under a seeded shuffle;
      rays/s and evaluations/s = (sum of steps + 5 x hits) / time;
  (b) for context, in the same run: sdfv_program_raymarch with aux of the same frame, and the host mirror
      (sdfv_program_raycast_host) on the CPUs this process may use, row order;
  (c) the wave utilisation of each order, sum(steps) / (64 x sum over waves of the wave's max steps), from the records' steps with
      tests/program_march_ref.lane_utilisation (a wave is 64 consecutive rays of the list).
There is one kernel: the list is cast one ray per lane in list order.  A persistent-wave form that refills finished lanes from
the list was not built; the utilisation under the shuffle says what it could gain at most.  Stamped with sdfv_build_id() and the
box."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
WIDTH, HEIGHT = 1920, 1080


def primary_rays(cam, width, height):
    """[height * width, 8] float32, pixel-row order: march_common.h's pixel_ray_raw, one float32 operation per step."""
    import numpy as np
    F = np.float32
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    px, py = xs.ravel().astype(F), ys.ravel().astype(F)
    ndc_x = ((px + F(0.5)) / F(width)) * F(2) - F(1)
    ndc_y = F(1) - ((py + F(0.5)) / F(height)) * F(2)
    sx = ndc_x * F(cam.aspect) * F(cam.tan_half_fovy)
    sy = ndc_y * F(cam.tan_half_fovy)
    r = np.zeros((height * width, 8), F)
    for a in range(3):
        r[:, a] = F(cam.eye[a])
        r[:, 4 + a] = F(cam.forward[a]) + F(cam.right[a]) * sx + F(cam.up[a]) * sy
    r[:, 7] = F(1e30)
    return r


def tile_order(width, height, tile=8):
    """The permutation that lists the pixels tile by tile (tiles row-major, a tile's pixels row-major)."""
    import numpy as np
    assert width % tile == 0 and height % tile == 0
    idx = np.arange(height * width).reshape(height // tile, tile, width // tile, tile)
    return np.ascontiguousarray(idx.transpose(0, 2, 1, 3)).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import program_march_ref as M
    import source_hash
    from program_mesh_bench import spheres8
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    assert torch.cuda.is_available(), "a measurement needs the device"

    builders = {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract(), "spheres8": spheres8(PM), "example_sixteen": PM.example_sixteen()}
    progs = {k: b.build() for k, b in builders.items()}
    rp = pkg.default_render_params(pkg.make_grid((256, 256, 256)))
    cam = pkg.camera_look_at(aspect=WIDTH / HEIGHT, eye=(1.9, 2.3, 3.8))
    rows = primary_rays(cam, WIDTH, HEIGHT)
    n = len(rows)
    orders = {"rows": np.arange(n), "tiles8x8": tile_order(WIDTH, HEIGHT), "shuffled": np.random.default_rng(20261021).permutation(n)}
    lists = {k: torch.from_numpy(np.ascontiguousarray(rows[p])).cuda() for k, p in orders.items()}
    hits = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "rays": n, "ops": {k: len(b.ops) for k, b in builders.items()},
           "kernels": ["sdfprog_cast"], "refill_kernel": "not built", "cast": {}}

    variants = {}
    for name, prog in progs.items():
        for order, rays in lists.items():
            variants[f"cast_{name}_{order}"] = (lambda prog=prog, rays=rays: prog.cast(rays, out=hits))
        variants[f"march_aux_{name}"] = (lambda prog=prog: prog.render(cam, WIDTH, HEIGHT, rp=rp, want_aux=True))
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():                  # alternated: every variant sees the same drift of clocks and neighbours
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t) * 1e3)
    stat = {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()}

    for name, prog in progs.items():
        entry = {"march_aux_1080p": stat[f"march_aux_{name}"]}
        for order, rays in lists.items():
            rec = PM.hits_view(prog.cast(rays, out=hits).cpu().numpy())
            steps, status = rec["steps"], rec["status"]
            s = dict(stat[f"cast_{name}_{order}"])
            evals = int(steps.sum()) + 5 * int((status == 1).sum())
            s.update({"hits": int((status == 1).sum()), "left_interval": int((status == -2).sum()), "out_of_steps": int((status == -1).sum()),
                      "off_the_box": int((status == 0).sum()), "sum_steps": int(steps.sum()), "max_steps": int(steps.max()),
                      "mrays_per_s": round(n / s["ms_median"] / 1e3, 2), "evaluations": evals,
                      "gevaluations_per_s": round(evals / s["ms_median"] / 1e6, 3),
                      "spread": round((s["ms_max"] - s["ms_min"]) / s["ms_median"], 4),
                      "wave_utilisation": round(M.lane_utilisation(steps.reshape(-1, 64), 64, 1), 4)})
            entry[order] = s
        if not args.no_host:
            t = time.perf_counter()
            prog.cast_host(rows)
            entry["host_mirror_rows_s"] = round(time.perf_counter() - t, 4)
            entry["host_threads"] = len(os.sched_getaffinity(0))
            entry["device_over_host_speedup_rows"] = round(entry["host_mirror_rows_s"] * 1e3 / entry["rows"]["ms_median"], 1)
        out["cast"][name] = entry
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
