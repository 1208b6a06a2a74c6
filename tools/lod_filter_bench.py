"""What a frame of a grid that is still loading costs under each filter (profiles/lod_filter.json is this tool's output).

    python tools/lod_filter_bench.py [--launches 30] [--warmup 5] [--out profiles/lod_filter.json]

1080p over the demo at 256^3.  Each mid-load state is produced the way a load produces it: sdfv_grid_init on a virgin grid, then
one sdfv_fill_grid_pass_ex with step L (L = 8, 4, 2), so the lattice of step L holds the demo and every other texel AIR_DIST.
Per state the two filters are alternated in ONE process -- SDFV_OPT_RAYMARCH_LOD_FILTER 0 (sdfSampleRawNearest, kMarchGeneral)
and 1 (the lattice filter, kMarchLattice) -- with device events around every launch; median, minimum and maximum per variant,
and the ratio lattice / nearest, whichever way it falls.  For context the loaded frame (lod 1) through the compiler's loop
(SDFV_RM_NO_ASM_LOOP) and through the default kernel.  Also per state: hits and summed steps of each filter's frame (the two
frames differ, so the two kernels do not do the same work).  Stamped with sdfv_build_id() and the box.  Reported, not gated."""
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
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lod_filter.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("sdf-viewer_amd")
    import source_hash
    K = pkg._capi
    W, H, N = 1920, 1080, 256
    prm = pkg.default_params()
    g = pkg.make_grid((N, N, N))
    cam = pkg.camera_look_at(aspect=W / H)
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "image": [W, H], "grid": [N, N, N], "launches": args.launches, "warmup": args.warmup, "states": {}}
    rgba = torch.empty((1, H, W, 4), dtype=torch.float32, device="cuda")

    def timed(variants):
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.launches):
            for k, fn in variants.items():  # alternated: every variant sees the same drift of clocks and neighbours
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)} for k, v in ms.items()}

    def march(rp, t0, t1, option, disable=0, **kw):
        with pkg.options({K.OPT_RAYMARCH_LOD_FILTER: option, K.OPT_RAYMARCH_DISABLE: disable}):
            return pkg.raymarch(rp, t0, t1, cam, W, H, **kw)

    for lod in (8, 4, 2):
        t0, t1 = pkg.alloc_textures(g)
        pkg.grid_init(g, t0, t1)                      # a virgin grid ...
        pkg.fill_grid_pass(prm, g, lod, t0, t1)       # ... after the pass with step `lod`
        torch.cuda.synchronize()
        rp = pkg.default_render_params(g)
        rp.lod_dist_between_samples = float(lod)
        stat = timed({"nearest": lambda: march(rp, t0, t1, 0, out=rgba), "lattice": lambda: march(rp, t0, t1, 1, out=rgba)})
        for name, option in (("nearest", 0), ("lattice", 1)):
            _, aux = march(rp, t0, t1, option, want_aux=True)
            a = aux[0].cpu().numpy().view(np.int32)
            stat[name].update(hits=int((a[..., 0] == 1).sum()), sum_steps=int(a[..., 1].sum()), max_steps=int(a[..., 1].max()))
        stat["lattice_over_nearest"] = round(stat["lattice"]["ms_median"] / stat["nearest"]["ms_median"], 4)
        stat["lattice_is_slower"] = stat["lattice_over_nearest"] > 1.0
        out["states"][f"lod{lod}"] = stat
        del t0, t1

    # context: the loaded grid
    t0, t1 = pkg.alloc_textures(g)
    dist = torch.empty((N, N, N), dtype=torch.float32, device="cuda")
    pkg.fill_grid(prm, g, t0, t1, dist=dist)
    torch.cuda.synchronize()
    rp = pkg.default_render_params(g)
    out["loaded"] = timed({"tex0_no_asm_loop": lambda: march(rp, t0, t1, 0, K.RM_NO_ASM_LOOP, out=rgba),
                           "dist_no_asm_loop": lambda: march(rp, t0, t1, 0, K.RM_NO_ASM_LOOP, out=rgba, dist=dist),
                           "dist_default": lambda: march(rp, t0, t1, 0, out=rgba, dist=dist)})
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
