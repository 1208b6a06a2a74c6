"""What an edit of an SDF program costs as a changed-box pass, against the dense fill it used to cost
(profiles/program_pass.json is this tool's output).

    python tools/program_pass_bench.py [--launches 24] [--sides 256,512] > profiles/program_pass.json

For `spheres8` (39 instructions, tools/program_mesh_bench.py) and `example_sixteen` (77), at each side, with the plain and with the
y-interleaved distance volume, over a grid LOADED with the program: the program with one operand edited is passed over it at step 1
(sdfv_program_grid_pass) with a centred changed box of 1/2, 1/4 and 1/8 of the side (1/8, 1/64 and 1/512 of the voxels), and
without a box (the scan alone, hinted SDFV_PASS_EXPECT_NOOP as the viewer hints it); beside them the dense fused fill of the
edited program (sdfv_program_fill_grid_commit), which is what the same edit cost before there was a pass.  All variants alternate
in ONE process after a warm-up, device events around every call, median and minimum per variant; each pass's ratio to the dense
fill, and the model "scan + dense * voxel share" next to what was measured.  Stamped with sdfv_build_id() and the box."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FRACTIONS = (2, 4, 8)


def edited(PM, builder, opcode, operand, value):
    """The builder's program with operand `operand` of its first `opcode` instruction set to `value`."""
    b = PM.Program(builder.bb)
    b.ops = list(builder.ops)
    at = next(i for i, (op, _) in enumerate(b.ops) if op == opcode)
    a = list(b.ops[at][1])
    a[operand] = float(value)
    b.ops[at] = (opcode, tuple(a))
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sides", default="256,512")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    K = pkg._capi
    import source_hash
    from program_mesh_bench import spheres8

    models = {"spheres8": (spheres8(PM), (K.OP_SPHERE, 0, 0.25)), "example_sixteen": (PM.example_sixteen(), (K.OP_TORUS, 1, 0.1))}
    out = {"build_id": pkg.lib.sdfv_build_id().decode(), "box": source_hash.box_uuid(), "device": torch.cuda.get_device_name(0),
           "launches": args.launches, "warmup": args.warmup, "step": 1,
           "changed_boxes": {f"1/{f}": [-1.0 / f] * 3 + [1.0 / f] * 3 for f in FRACTIONS}, "results": {}}
    for side in [int(s) for s in args.sides.split(",")]:
        g = pkg.make_grid((side, side, side))
        t0, t1 = pkg.alloc_textures(g)
        dist = torch.empty((side, side, side), device="cuda")
        for name, (builder, edit) in models.items():
            loaded, prog = builder.build(), edited(PM, builder, *edit).build()
            for layout, lflag in (("plain", 0), ("interleaved", K.PASS_VOLUME_INTERLEAVED)):
                loaded.fill_grid(g, t0, t1, dist=dist, flags=lflag)
                variants = {"dense_fill": lambda: prog.fill_grid(g, t0, t1, dist=dist, flags=lflag)}
                for f in FRACTIONS:
                    box = [-1.0 / f] * 3 + [1.0 / f] * 3
                    variants[f"box_1/{f}"] = lambda box=box: prog.grid_pass(g, 1, t0, t1, dist=dist, changed_box=box, flags=lflag)
                variants["scan_no_box"] = lambda: prog.grid_pass(g, 1, t0, t1, dist=dist, flags=lflag | K.PASS_EXPECT_NOOP)
                for _ in range(args.warmup):
                    for fn in variants.values():
                        fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in variants}
                for _ in range(args.launches):
                    for k, fn in variants.items():      # alternated: every variant sees the same drift of clocks and neighbours
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        ms[k].append(e0.elapsed_time(e1))
                res = {k: {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)}
                       for k, v in ms.items()}
                dense, scan = res["dense_fill"]["ms_median"], res["scan_no_box"]["ms_median"]
                for f in FRACTIONS:
                    r = res[f"box_1/{f}"]
                    r["voxel_share"] = 1.0 / f ** 3
                    r["over_dense_fill"] = round(r["ms_median"] / dense, 4)
                    r["model_scan_plus_share_ms"] = round(scan + dense / f ** 3, 5)
                res["scan_no_box"]["over_dense_fill"] = round(scan / dense, 4)
                out["results"][f"{name}/{side}/{layout}"] = dict(instructions=len(builder.ops), **res)
        del t0, t1, dist
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
