"""CPU tests of dual contouring (include/sdfgrid.h, "Dual contouring"; SDFV_MESHER_DUAL_CONTOURING_PARTICLE = 4): what the entry
points accept and refuse without a device, the sanity of the numpy restatement the GPU tests compare against
(tests/mesh_ref.py through tests/program_mesh_ref.py and tests/demo_mesh_ref.py) on geometry whose answer is known, and what the built kernels look like.  No device needed."""
import ctypes as C
import functools
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import demo_mesh_ref as DM
import mesh_ref as MR
import program_mesh_ref as M
import program_ref as R
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

INVALID, NO_DEVICE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def test_the_constant_is_the_reference_algorithm_number(pkg):
    assert pkg.MESHER_DUAL_CONTOURING_PARTICLE == pkg._capi.MESHER_DUAL_CONTOURING_PARTICLE == MR.DUAL == 4
    assert pkg.MESHER_MARCHING_CUBES == 0
    header = open(os.path.join(ROOT, "include", "sdfgrid.h")).read()
    assert re.search(r"#define SDFV_MESHER_DUAL_CONTOURING_PARTICLE 4u\b", header)


def test_algorithm_4_is_accepted_and_the_other_meshers_are_still_refused(pkg, PM):
    """Without a device algorithm 4 passes every argument check and stops at SDFV_ERR_NO_DEVICE (with one it would mesh: the GPU
    tests); 1, 2, 3 and 5 are "Unsupported algorithm" either way, and limit and flag errors are still reported."""
    lib, K = pkg.lib, pkg._capi
    prog = R.catalogue(PM)["anchor"].build()
    lo, hi = pkg.f3((-1, -1, -1)), pkg.f3((1, 1, 1))
    m = K.Mesh()

    def extract(n=8, algorithm=4, flags=0, lo=lo, hi=hi):
        m.vertices, m.indices, m.n_vertices, m.n_indices = 1, 1, 7, 7
        rc = lib.sdfv_program_mesh_extract(prog.h, lo, hi, n, algorithm, flags, C.byref(m), None)
        return rc, lib.sdfv_last_error()

    for algorithm in (1, 2, 3, 5, 0xffffffff):
        rc, msg = extract(algorithm=algorithm)
        assert rc == INVALID and b"Unsupported algorithm" in msg, (algorithm, msg)
        prm = pkg.default_params()
        assert lib.sdfv_mesh_extract(C.byref(prm), 0, lo, hi, 8, algorithm, C.byref(m), None) == INVALID
        assert b"Unsupported algorithm" in lib.sdfv_last_error()
    for n in (0, 1025):
        rc, msg = extract(n=n)
        assert rc == INVALID and b"outside [1, 1024]" in msg, (n, msg)
    for flags in (2, 3, 0x80000000):
        rc, msg = extract(flags=flags)
        assert rc == INVALID and b"unknown flags" in msg, (flags, msg)
    rc, msg = extract(lo=None)
    assert rc == INVALID and b"both" in msg
    if lib.sdfv_device_count() == 0:
        for flags in (0, K.MESH_WITH_MATERIALS):
            rc, msg = extract(flags=flags)
            assert rc == NO_DEVICE and b"no HIP device" in msg, (rc, msg)
            assert (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)
        prm = pkg.default_params()
        assert lib.sdfv_mesh_extract(C.byref(prm), 0, lo, hi, 8, 4, C.byref(m), None) == NO_DEVICE
        assert lib.sdfv_mesh_extract(C.byref(prm), 0, lo, hi, 0, 4, C.byref(m), None) == INVALID
    assert lib.sdfv_abi_version() == 5     # no new export: the version stays


def test_cpp_host_refuses_host_only_surfaces_and_the_two_other_meshers(tmp_path):
    """tests/c/dual_contour_host.cpp host-only, linked against the product library: mesh_sdf with the new mesher answers "no
    device form" for a surface that has none, and the QEF and linear-hashed variants are still "Unsupported algorithm"."""
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "dual_contour_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(lib, "host"),
                           os.path.join(ROOT, "tests", "c", "dual_contour_host.cpp"), "-o", str(exe), "-L", lib, "-lsdfviewer_host",
                           "-lsdfgrid", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                           "-Wl,-rpath," + lib, "-ldl", "-pthread"])
    r = subprocess.run([str(exe), "host-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dual_contour_host host-only ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- the restatement against geometry: it is the yardstick of tests/test_gpu_dual_contour.py ----
@functools.lru_cache(maxsize=None)
def restated(kind, size, n):
    v, i, s = M.extract(M.primitive(kind, size), n, BOX, algorithm=MR.DUAL)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i, s


def test_the_hermite_records_are_the_marching_cubes_vertices(PM):
    """The restatement's own edge positions equal tests/program_mesh_ref.py's marching-cubes vertices bit for bit, and so do the
    normals: the Hermite data is what is already pinned."""
    b = R.catalogue(PM)["deep"]
    mv, _, _ = M.extract(b.ops, 12, b.bb)
    _, _, s = M.extract(b.ops, 12, b.bb, algorithm=MR.DUAL)
    assert mv.shape[0] == 173 and (M.bits(mv[:, :6]) == M.bits(s["hermite"])).all()


def test_a_cube_keeps_its_creases_and_corners():
    """CUBE 0.6 in the box +-1 at 12 cells (cell side 1/6, faces at 0.6 = 3.6 cells: no lattice plane lies on a face).  The
    tolerance 1e-4: the corner residual (2/3)^24 * (cell diagonal 0.29) = 1.7e-5, plus the finite-difference normal's tilt (under
    1e-5) times a lever arm of 0.1.  A marching-cubes-style placement (vertices on lattice edges) has no vertex on a crease at
    all and fails the 72 / 8 counts outright."""
    v, i, s = restated("cube", 0.6, 12)
    assert len(s["hermite"]) == 294 and v.shape[0] == 296 and i.shape[0] == 3 * 588 and s["quads"] == 294
    on = np.abs(np.abs(v[:, :3].astype(np.float64)) - 0.6) <= 1e-4
    assert (on.sum(axis=1) == 2).sum() == 72, "crease vertices: 12 edges of the cube x 6 cells"
    assert (on.sum(axis=1) == 3).sum() == 8, "corner vertices"
    worst = np.abs(np.abs(v[:, :3].astype(np.float64)).max(axis=1) - 0.6).max()
    print("cube 0.6 at 12 cells: worst distance from the surface", worst)
    assert worst <= 1e-4
    assert (s["used"] == s["edges"]).all() and s["edges"].min() >= 3


@pytest.mark.parametrize("n", [5, 9, 12])
def test_a_sphere_stays_within_the_second_order_bound(n):
    """SPHERE 0.6: the tangent planes of a cell's edges meet within sagitta distance of the sphere: |r - 0.6| <= cell^2 / (2 * 0.6)."""
    v, i, _ = restated("sphere", 0.6, n)
    cell = 2.0 / n
    worst = np.abs(np.linalg.norm(v[:, :3].astype(np.float64), axis=1) - 0.6).max()
    print("sphere 0.6 at", n, "cells: worst |r - 0.6|", worst, "bound", cell * cell / 1.2)
    assert v.shape[0] > 0 and worst <= cell * cell / (2 * 0.6)


@pytest.mark.parametrize("kind,size,n", [("cube", 0.6, 12), ("sphere", 0.6, 5), ("sphere", 0.6, 9), ("sphere", 0.6, 12)])
def test_restated_meshes_are_closed_and_face_outward(kind, size, n):
    v, i, _ = restated(kind, size, n)
    assert i.min() == 0 and i.max() == v.shape[0] - 1 and len(np.unique(i)) == v.shape[0]
    MR.assert_closed_and_oriented(i)
    tri = v[i.reshape(-1, 3), :3].astype(np.float64)
    face_n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    solid = np.linalg.norm(face_n, axis=1) > 1e-12                     # a quad on a crease may fold one triangle to a line
    assert solid.sum() > len(tri) // 2
    centroid = tri.mean(axis=1)
    if kind == "sphere":
        outward = centroid
    else:                                                             # the cube's outward direction: the dominant axis
        outward = np.zeros_like(centroid)
        a = np.abs(centroid).argmax(axis=1)
        outward[np.arange(len(a)), a] = np.sign(centroid[np.arange(len(a)), a])
    assert (np.einsum("ij,ij->i", face_n, outward)[solid] > 0).all()


def test_the_restated_demo_is_closed(oracle):
    """The demo (cube 0.95 - sphere 1.05) at 24 cells, from the oracle's distances and normals."""
    prm = oracle.default_params()
    v, i, s = DM.extract_demo(oracle, prm, 24, ((-1, -1, -1), (1, 1, 1)), algorithm=MR.DUAL)
    assert v.shape[0] == 4528 and i.shape[0] == 3 * 9072
    MR.assert_closed_and_oriented(i)
    assert np.isfinite(v).all()


# ---- the built kernels (tests/kernel_objects.py) ----
DC_KERNELS = ("dc_cell_count", "dc_edge_count", "dc_totals", "dc_cell_list", "dc_solve", "dc_quads")
NEW_KERNELS = DC_KERNELS + ("mesh_demo_normals",)        # the demo's per-vertex kernel (mesh_kernels.hip)


def interpreter_loops(table, name):
    """Backward branches of a kernel whose span holds the eighteen instruction bodies and a wide scalar load: the test of
    tests/test_program_mesh_cpu.py for "this is the interpreter"."""
    ins = []
    for ln in disassembly(table[name]["co"], name).split("\n"):
        mm = re.match(r"\s+(\S+)[^/]*//\s*([0-9A-Fa-f]{12}):[^<]*(?:<[^>+]*\+0x([0-9a-f]+)>)?", ln)
        if mm:
            ins.append((mm.group(1), int(mm.group(2), 16), None if mm.group(3) is None else int(mm.group(3), 16)))
    base = ins[0][1]
    back = [(base + to, at) for o, at, to in ins if o.startswith(("s_cbranch", "s_branch")) and to is not None and base + to < at]
    loops = []
    for lo, hi in back:
        body = [o for o, at, _ in ins if lo <= at <= hi]
        if len(body) > 200 and any(re.match(r"s_load_dwordx(4|8|16)$", o) for o in body):
            loops.append(body)
    return loops


def test_dual_contour_kernels_keep_the_resource_ceilings(code_objects):
    """every new kernel without scratch and without spills, at most 64 VGPRs (8 waves per SIMD, the step the measured
    counts -- 50 for dc_solve, 18 or fewer for the others -- sit on).  None of them contains an interpreter loop; the kernels that
    do and that dual contouring runs over its solved vertices (sdfprog_mesh_vertices[_mat]) keep theirs free of vector-memory
    and LDS operations."""
    table = kernel_table(code_objects)
    assert sorted(n for n in table if n.startswith("dc_")) == sorted(DC_KERNELS)
    for name in NEW_KERNELS:
        k = table[name]
        print(name, {a: b for a, b in k.items() if a != "co"})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] <= 64, (name, k)
        assert k["kernarg"] <= 256, (name, k)
        ops = [ln.split("//")[0].split()[0] for ln in disassembly(k["co"], name).split("\n") if ln.split("//")[0].split()]
        assert not any(o.startswith(("scratch_", "buffer_", "ds_")) for o in ops), name
        assert not interpreter_loops(table, name), (name, "no program is interpreted here")
    for name in ("sdfprog_mesh_vertices", "sdfprog_mesh_vertices_mat"):
        loops = interpreter_loops(table, name)
        assert loops, (name, "no interpreter loop found")
        inner = min(loops, key=len)
        assert not any(o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_")) for o in inner), name
