"""GPU tests of SDF programs: the point sampler and the dense fill of sdfv_program_* against the numpy restatement of the header's
table (tests/program_ref.py), the demo anchor on the device, a program loaded through the viewer against the oracle's loop, and
the plain-C path.  Every comparison is bitwise (but for the test of non-finite points: a NaN distance there is compared as a NaN,
include/sdfgrid.h leaves its payload and sign open)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import program_ref as R
from program_fill_check import fill_equals_packing, same_bits, voxel_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def V(pkg):
    return importlib.import_module("sdf-viewer_amd.viewer")


@pytest.mark.timeout(600)
def test_sample_points_equals_the_numpy_restatement_bitwise(pkg, PM):
    pts = R.points()
    nan_records = 0
    dev = torch.from_numpy(pts).cuda()
    for name, builder in R.catalogue(PM).items():
        prog = builder.build()
        for distance_only in (False, True):
            want = R.run(builder.ops, pts, distance_only)
            nan_records += int(np.isnan(want[:, 0]).sum())
            same_bits(prog.sample_points(dev, distance_only).cpu().numpy(), want, f"{name} device buffers d_only={distance_only}")
            same_bits(prog.sample_points_host(pts, distance_only), want, f"{name} host buffers d_only={distance_only}")
            for n in (1, 255, 257, 1000):                    # the scalar kernel alone, both kernels, an unaligned start
                same_bits(prog.sample_points(dev[:n].contiguous(), distance_only).cpu().numpy(), want[:n], f"{name} n={n}")
            off = dev[3:3 + 512].clone()                     # 512 points whose buffer is not 16-byte aligned: no staged form
            flat = torch.empty(3 * 512 + 1, device="cuda")
            flat[1:] = off.reshape(-1)
            view = flat[1:].view(512, 3)
            assert view.data_ptr() % 16 != 0
            same_bits(prog.sample_points(view, distance_only).cpu().numpy(), want[3:3 + 512], f"{name} unaligned")
        assert prog.sample_points(dev[:0].contiguous()).shape == (0, 7)
        assert pkg.lib.sdfv_program_sample_points(prog.h, None, 0, 0, None, None) == 0
    assert 0 < nan_records < len(pts)                        # the huge points do make NaNs (inf - inf) in some program


@pytest.mark.timeout(600)
def test_sample_points_on_rows_where_a_wave_holds_many_materials(pkg, PM):
    """The rows of the 256 x 6 x 4 grid fed to the samplers in order: `envelope` puts 64 distinct material indices into a wave,
    `late_material` mixes lanes without an index with lanes that have one.  More than 256 points 16-byte aligned (the staged
    kernel, then the scalar tail), a ragged batch and an unaligned one (the scalar kernel alone)."""
    dims, bb_min, bb_max = R.ROW_GRID
    pos = voxel_positions(dims, bb_min, bb_max)
    dev = torch.from_numpy(pos).cuda()
    flat = torch.empty(3 * 1000 + 1, device="cuda")
    flat[1:] = dev[64:1064].reshape(-1)
    unaligned = flat[1:].view(1000, 3)
    assert dev.data_ptr() % 16 == 0 and unaligned.data_ptr() % 16 != 0 and len(pos) > 256 and len(pos[:-57]) % 256
    for name in ("envelope", "late_material"):
        builder = R.catalogue(PM)[name]
        prog = builder.build()
        if name == "envelope":
            want = R.assert_envelope_stresses(builder.ops, pos, dims[0])
        else:
            want = R.assert_late_material_stresses(builder.ops, pos, dims[0])
        same_bits(prog.sample_points(dev).cpu().numpy(), want, f"{name} rows, aligned")
        same_bits(prog.sample_points(dev[:-57].contiguous()).cpu().numpy(), want[:-57], f"{name} rows, aligned with a tail")
        same_bits(prog.sample_points(dev[64:64 + 191].contiguous()).cpu().numpy(), want[64:64 + 191], f"{name} rows, ragged")
        same_bits(prog.sample_points(unaligned).cpu().numpy(), want[64:1064], f"{name} rows, unaligned")
        same_bits(prog.sample_points_host(pos), want, f"{name} rows, host buffers")
        same_bits(prog.sample_points(dev, True).cpu().numpy(), R.run(builder.ops, pos, True), f"{name} rows, distance only")


@pytest.mark.timeout(600)
def test_non_finite_and_extreme_points_on_the_device(pkg, PM, V):
    """+-inf, NaN, +-3e38 and subnormal coordinates among ordinary points of the same waves, through the device sampler with
    device and with host buffers and through the host callbacks: ordinary input handling.  The calls return, and the header's
    rule for NaN results holds (R.assert_records_under_the_nan_rule)."""
    pts, ordinary = R.odd_batch()
    dev = torch.from_numpy(pts).cuda()
    for name in ("all_ops", "envelope"):
        builder = R.catalogue(PM)[name]
        prog = builder.build()
        surf = prog.as_surface()
        s = surf.struct
        for distance_only in (False, True):
            want, decided = R.run(builder.ops, pts, distance_only, want_decided=True)
            what = f"{name} d_only={distance_only}"
            R.assert_records_under_the_nan_rule(prog.sample_points(dev, distance_only).cpu().numpy(), want, decided, ordinary, what + " device")
            R.assert_records_under_the_nan_rule(prog.sample_points_host(pts, distance_only), want, decided, ordinary, what + " host buffers")
            n = 1001                                         # the scalar kernel alone on part of it
            R.assert_records_under_the_nan_rule(prog.sample_points(dev[:n].contiguous(), distance_only).cpu().numpy()[:n], want[:n],
                                                decided[:n], ordinary[:n], what + " ragged")
            out = np.full((len(pts), 7), np.nan, np.float32)
            assert s.sample_batch(s.user, pts.ctypes.data_as(V.FP), len(pts), int(distance_only), out.ctypes.data_as(C.POINTER(V.Sample))) == 0
            R.assert_records_under_the_nan_rule(out, want, decided, ordinary, what + " host callbacks")
        torch.cuda.synchronize()


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("dims", [(9, 7, 5), (64, 64, 64), (250, 130, 66), (256, 256, 256), R.ROW_GRID[0]])
def test_fill_equals_packing_the_numpy_samples_bitwise(pkg, PM, dims):
    names = ("all_ops",) if dims[0] * dims[1] * dims[2] > 1 << 22 else ("all_ops", "deep", "anchor", "no_material", "envelope",
                                                                        "late_material")
    fill_equals_packing(pkg, PM, dims, (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8), names)


@pytest.mark.timeout(600)
def test_fill_of_the_envelope_on_one_wave_per_row_bitwise(pkg, PM):
    """`envelope` on a 64-wide grid over the x-range of its touch points: the tx64 kernels see 64 distinct materials in a wave."""
    bb_min, bb_max = R.envelope_box_64()
    fill_equals_packing(pkg, PM, R.ENVELOPE_GRID_64, bb_min, bb_max, ("envelope",))


@pytest.mark.timeout(600)
def test_the_demo_as_a_program_fills_the_demo_distance(pkg, PM):
    """CUBE 0.95, SPHERE 1.05, SUBTRACT at 256^3: tex0.r of the program fill == tex0.r of sdfv_fill_grid, every voxel."""
    dims = (256, 256, 256)
    grid = pkg.make_grid(dims)
    prog = R.catalogue(PM)["anchor"].build()
    p0, p1 = pkg.alloc_textures(grid)
    d0, d1 = pkg.alloc_textures(grid)
    prog.fill_grid(grid, p0, p1)
    pkg.fill_grid(pkg.default_params(), grid, d0, d1)
    torch.cuda.synchronize()
    assert bool((p0[..., 0].contiguous().view(torch.int32) == d0[..., 0].contiguous().view(torch.int32)).all())
    assert 0.0 < float((p0[..., 0] < 0.1).float().mean()) < 1.0


def reference_sampler(oracle, ops, dims, bb):
    """An or_sample_fn over the numpy restatement: every voxel position of the grid evaluated once, looked up by position."""
    pos = voxel_positions(dims, bb[:3], bb[3:])
    rec = R.run(ops, pos)
    table = {pos[i].tobytes(): rec[i] for i in range(len(pos))}

    @oracle.SAMPLE_FN
    def ref_sample(_user, p, _distance_only, out):
        s = table[np.array([p[0], p[1], p[2]], np.float32).tobytes()]
        for i in range(7):
            out[i] = s[i]
    return ref_sample


@pytest.mark.timeout(900)
@pytest.mark.parametrize("dims,layout", [((24, 18, 20), 1), ((24, 18, 20), 2), ((21, 17, 11), 1)])
def test_a_program_loads_through_the_viewer_like_the_oracle_loop(pkg, PM, V, oracle, dims, layout):
    builder = R.catalogue(PM)["all_ops"]
    bb = builder.bb
    prog = builder.build()
    surf = prog.as_surface()
    assert surf.struct.sample_batch_device
    v = V.Viewer.new_voxels(dims, bb, 3, layout=layout)
    stream = torch.cuda.Stream()
    v.set_stream(stream.cuda_stream)
    r0, r1 = oracle.grid_init(dims)
    lm = oracle.lm_new(dims, 3)
    ref_sample = reference_sampler(oracle, builder.ops, dims, bb)
    calls = 0
    while v.state()["remaining"]:
        n = v.update(surf, budget_ns=0)        # one run per call: every intermediate state is compared
        assert n > 0
        assert oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, max_iterations=n, bb_min=bb[:3], bb_max=bb[3:]) == n
        t0, t1 = v.download()
        same_bits(t0, r0, f"{dims} layout {layout} call {calls} tex0")
        same_bits(t1, r1, f"{dims} layout {layout} call {calls} tex1")
        calls += 1
    assert calls >= 3 and v.state()["lod"] == 1.0
    v.close()


@pytest.mark.timeout(900)
def test_device_route_host_route_and_dense_fill_agree_at_96x80x72(pkg, PM, V):
    dims = (96, 80, 72)
    builder = R.catalogue(PM)["all_ops"]
    bb = builder.bb
    prog = builder.build()
    grid = pkg.make_grid(dims, bb[:3], bb[3:])
    f0, f1 = pkg.alloc_textures(grid)
    prog.fill_grid(grid, f0, f1)
    torch.cuda.synchronize()
    loaded = {}
    for route in ("device", "host"):
        surf = prog.as_surface(device_route=route == "device")
        assert bool(surf.struct.sample_batch_device) == (route == "device")
        v = V.Viewer.new_voxels(dims, bb, 3)
        while v.state()["remaining"]:
            assert v.update(surf, budget_s=0.03) > 0
        v.commit()
        loaded[route] = v.download()
        if route == "device":
            view = V.View((C.c_float * 3)(2.5, 3.0, 5.0), (C.c_float * 3)(0.0, 0.0, 0.0), (C.c_float * 3)(0.0, 1.0, 0.0), 45.0, 0.1, 1000.0)
            frame = v.render(160, 120, view).cpu().numpy()
        v.close()
    for route in loaded:
        same_bits(loaded[route][0], f0.cpu().numpy(), f"{route} route tex0 vs the dense fill")
        same_bits(loaded[route][1], f1.cpu().numpy(), f"{route} route tex1 vs the dense fill")
    # a frame from the viewer == a frame from the dense-filled textures (the same camera, the viewer's default uniforms)
    rp = pkg.default_render_params(grid)
    cam = pkg.camera_look_at(aspect=160 / 120)
    want = pkg.raymarch(rp, f0, f1, cam, 160, 120)[0].cpu().numpy()
    same_bits(frame, want, "a frame of the loaded viewer vs one of the dense fill")
    assert float(np.abs(want[..., :3]).max()) > 0.0


@pytest.mark.timeout(900)
def test_cpp_program_sdf_loads_through_the_cpp_viewer(pkg, PM, host):
    """A C++ ProgramSDF handed to the C++ SDFViewer::update (no C surface in between): the class's device sampler loads the
    grid to the bits of the dense fill."""
    host.H.sdfvh_program_sdf_new.restype, host.H.sdfvh_program_sdf_new.argtypes = C.c_void_p, [C.c_void_p]
    host.H.sdfvh_sdf_has_device_sampler.restype, host.H.sdfvh_sdf_has_device_sampler.argtypes = C.c_int, [C.c_void_p]
    dims = (40, 36, 28)
    builder = R.catalogue(PM)["all_ops"]
    prog = builder.build()
    sdf = host.SDF(host.H.sdfvh_program_sdf_new(prog.h))
    assert host.H.sdfvh_sdf_has_device_sampler(sdf.h) == 1
    v = host.Viewer.new_voxels(dims, builder.bb, 3)
    calls = 0
    while v.remaining():
        assert v.update(sdf, 0.03) > 0, v.last_error()
        calls += 1
        assert calls < 10000
    t0, t1 = v.download()
    grid = pkg.make_grid(dims, builder.bb[:3], builder.bb[3:])
    f0, f1 = pkg.alloc_textures(grid)
    prog.fill_grid(grid, f0, f1)
    torch.cuda.synchronize()
    same_bits(t0, f0.cpu().numpy(), "ProgramSDF through SDFViewer::update tex0 vs the dense fill")
    same_bits(t1, f1.cpu().numpy(), "ProgramSDF through SDFViewer::update tex1 vs the dense fill")
    del v, sdf


@pytest.mark.timeout(900)
def test_plain_c_program_fills_and_loads(tmp_path):
    """tests/c/program_smoke.c: C11, no C++ and no Python between the caller and the libraries."""
    exe = tmp_path / "program_smoke"
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c", "program_smoke.c"), "-o", str(exe), "-L", lib,
           "-lsdfviewer_host", "-lsdfgrid", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "program_smoke ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
