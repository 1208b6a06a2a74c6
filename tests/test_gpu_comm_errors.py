"""What the slab communicator answers to bad arguments once a communicator is alive: the status code and the exact
sdfv_last_error() text of every argument check of sdfv_slab_* / sdfv_comm_* / sdfv_bands_scatter that sits behind a live handle
or behind the device test, and, where a call violates two rules, which one it reports.  tests/golden/comm_errors.json holds the
library's answers as recorded from it on a GPU (`python tests/test_gpu_comm_errors.py --record`); the test replays every case and
compares code and text exactly.  tests/test_api_errors_cpu.py holds the checks that need neither.

Every refusal returns before anything is enqueued: no case launches a kernel or posts a message.  Buffers are small real
allocations; the misaligned ones are addresses inside them.  The two rows that answer 0 are calls with nothing to do (no cameras;
they pin that a scratch block nobody needs may be NULL).  A world of one cannot reach two of the layer's texts: the gathering rank
needs no scratch (there are no peers), so "scratch: ..." of sdfv_comm_gather_bands is not recorded, and z_bounds that decrease
cannot also run from 0 to the depth, so that row pins the ORDER of the two z_bounds rules instead."""
import ctypes as C
import importlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "comm_errors.json")
ANSWERS_ZERO = ("comm_gather_bands/scratch_null_unneeded_is_ok", "comm_gather_bands/scratch_null_unneeded_with_bytes_is_ok")


def build_cases(pkg, loop, loop2, line):
    """[(name, thunk)] over loop / loop2 (periodic worlds of one, upper halo 1 / 2) and line (non-periodic world of one)."""
    lib = pkg.lib
    cases, keep = [], []

    def case(name, fn, *args):
        assert name not in [n for n, _ in cases], name
        cases.append((name, lambda: getattr(lib, fn)(*args)))

    def buf(n_floats):
        t = torch.zeros(n_floats, dtype=torch.float32, device="cuda")
        keep.append(t)
        return t.data_ptr()

    def grid(dims=(4, 4, 4), z=None):
        g = pkg.make_grid(dims, z_begin=z[0] if z else 0, z_end=z[1] if z else None)
        keep.append(g)
        return C.byref(g)

    T0, T1, D = buf(7 * 64), buf(7 * 64), buf(7 * 16)   # 4 x 4 slices: 4 owned + 1 ghost below + up to 2 above
    prm = pkg.default_params()
    keep.append(prm)
    P, G = C.byref(prm), grid()
    EMPTY, BEYOND, FLAT, THIN = grid(z=(2, 2)), grid(z=(3, 9)), grid((4, 0, 4)), grid(z=(1, 2))

    # ---- the slab checks of the step and of the exchange alone
    def slab(name, comm=loop, g=G, tex0=T0, tex1=T1, dist=None):
        if dist is None:
            case(f"slab_halo_exchange/{name}", "sdfv_slab_halo_exchange", comm.handle, g, tex0, tex1, None)
            case(f"slab_fill_step/{name}", "sdfv_slab_fill_step", comm.handle, P, 0, g, tex0, tex1, None)
        case(f"slab_fill_step_commit/{name}", "sdfv_slab_fill_step_commit", comm.handle, P, 0, g, tex0, tex1, D if dist is None else dist, None)

    slab("grid_null", g=None)
    slab("tex1_null", tex1=None)
    slab("tex0_by4", tex0=T0 + 4)
    slab("empty", g=EMPTY)
    slab("beyond_depth", g=BEYOND)
    slab("dims0", g=FLAT)
    slab("thin_for_halo2", comm=loop2, g=THIN)
    slab("dist_by2", dist=D + 2)
    slab("tex_null+beyond_depth", tex0=None, g=BEYOND)
    slab("tex_by4+empty", tex1=T1 + 4, g=EMPTY)
    slab("thin_for_halo2+dist_by2", comm=loop2, g=THIN, dist=D + 2)

    # ---- the gathers (a world of one: rank 0 is the only dst)
    PART, OUT = buf(8 * 8 * 4), buf(8 * 8 * 4)

    def bands(name, part=PART, band_height=16, n_cameras=1, channels=4, dst=0, out=OUT, scratch=None, scratch_bytes=0):
        case(f"comm_gather_bands/{name}", "sdfv_comm_gather_bands", loop.handle, part, band_height, n_cameras, 8, 8, channels, dst, out,
             scratch, scratch_bytes, None)

    bands("dst_negative", dst=-1)
    bands("dst1", dst=1)
    bands("channels0", channels=0)
    bands("band_height5", band_height=5)
    bands("part_null", part=None)
    bands("out_null", out=None)
    bands(ANSWERS_ZERO[0].split("/")[1], part=None, n_cameras=0)
    bands(ANSWERS_ZERO[1].split("/")[1], part=None, n_cameras=0, scratch_bytes=4096)
    bands("dst1+channels0", dst=1, channels=0)
    bands("channels0+band_height5", channels=0, band_height=5)
    fn = "sdfv_comm_gather_cameras"
    case("comm_gather_cameras/dst1", fn, loop.handle, PART, 1, 8, 8, 4, 1, OUT, None)
    case("comm_gather_cameras/part_null", fn, loop.handle, None, 1, 8, 8, 4, 0, OUT, None)
    case("comm_gather_cameras/out_null", fn, loop.handle, PART, 1, 8, 8, 4, 0, None, None)
    dims3 = (C.c_uint32 * 3)(4, 4, 4)
    keep.append(dims3)

    def slabs(name, dims=dims3, z=(0, 4), tex0=T0, dist_owned=None, out_dist=None):
        zb = None if z is None else (C.c_uint32 * 2)(*z)
        keep.append(zb)
        case(f"comm_allgather_slabs/{name}", "sdfv_comm_allgather_slabs", loop.handle, dims, zb, tex0, T1, dist_owned, OUT, OUT, out_dist, None)

    slabs("dims_null", dims=None)
    slabs("z_bounds_null", z=None)
    slabs("tex_null", tex0=None)
    slabs("dist_owned_alone", dist_owned=D)
    slabs("out_dist_alone", out_dist=D)
    slabs("z_bounds_from1", z=(1, 4))
    slabs("z_bounds_to3", z=(0, 3))
    slabs("z_bounds_decreasing", z=(4, 0))
    case("bands_scatter/band_height5", "sdfv_bands_scatter", PART, 0, 1, 5, 1, 8, 8, 4, OUT, None)

    # ---- the sharded march
    g_march = pkg.make_grid((4, 4, 4))
    rp, cam = pkg.default_render_params(g_march), pkg.camera_look_at(aspect=1.0)
    keep.extend([g_march, rp, cam])
    need = int(lib.sdfv_slab_march_scratch_bytes(16))
    SCRATCH, STATUS, RGBA = buf(need // 4 + 4), buf(4), buf(8 * 8 * 4)

    def march(name, comm=line, scratch=SCRATCH, scratch_bytes=need, capacity=16, flags=0, status=STATUS):
        case(f"slab_march/{name}", "sdfv_slab_march", comm.handle, C.byref(rp), C.byref(g_march), T0, T1, C.byref(cam), 8, 8, RGBA, None,
             scratch, scratch_bytes, capacity, flags, status, None)

    march("periodic", comm=loop)
    march("scratch_null", scratch=None)
    march("status_null", status=None)
    march("flags", flags=0x80)
    march("capacity0", capacity=0)
    march("scratch_by4", scratch=SCRATCH + 4, scratch_bytes=need)
    march("scratch_one_byte_short", scratch_bytes=need - 1)
    march("flags+capacity0", flags=0x80, capacity=0)
    return cases, keep  # (keep: the buffers and structs the thunks point into)


def run_cases(pkg):
    par = importlib.import_module("sdf-viewer_amd.parallel")
    comms = [par.SlabComm(pkg, 0, 1, periodic=True), par.SlabComm(pkg, 0, 1, periodic=True, halo_hi=2), par.SlabComm(pkg, 0, 1)]
    try:
        cases, keep = build_cases(pkg, *comms)
        got = {}
        for name, thunk in cases:
            code = thunk()
            got[name] = {"code": code, "error": pkg.lib.sdfv_last_error().decode() if code else ""}  # (0 leaves the last message be)
        torch.cuda.synchronize()
        del keep
        return got
    finally:
        for c in comms:
            c.close()


def test_every_communicator_check_answers_with_the_recorded_code_and_text(pkg):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = run_cases(pkg)
    assert sorted(got) == sorted(want)
    # every row is a refusal of the arguments (-1), but for the calls with nothing to do
    assert all(v["code"] == -1 for k, v in want.items() if k not in ANSWERS_ZERO)
    assert all(want[k] == {"code": 0, "error": ""} for k in ANSWERS_ZERO)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, "w") as f:
        json.dump(run_cases(importlib.import_module("sdf-viewer_amd")), f, indent=0, sort_keys=True)
        f.write("\n")
