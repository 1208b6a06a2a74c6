"""CPU tests of meshing over SDF programs (include/sdfgrid.h, "SDF programs: meshing"): what the four entry points refuse, with
their messages; what the built kernels look like; and the sanity of the numpy restatement the GPU tests compare against
(tests/program_mesh_ref.py over tests/mesh_ref.py).  No device needed."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import mesh_ref as MR
import program_mesh_ref as M
import program_ref as R
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

INVALID, NO_DEVICE = -1, -4


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def test_argument_errors_come_first_and_without_a_device_nothing_is_written(pkg, PM):
    lib, K = pkg.lib, pkg._capi
    prog = R.catalogue(PM)["anchor"].build()
    lo, hi = pkg.f3((-1, -1, -1)), pkg.f3((1, 1, 1))
    m = K.Mesh()

    def extract(p=prog.h, lo=lo, hi=hi, n=8, algorithm=0, flags=0, out=m):
        m.vertices, m.indices, m.n_vertices, m.n_indices = 1, 1, 7, 7
        rc = lib.sdfv_program_mesh_extract(p, lo, hi, n, algorithm, flags, None if out is None else C.byref(out), None)
        return rc, lib.sdfv_last_error()

    assert extract(out=None) == (INVALID, b"out is NULL")
    rc, msg = extract(p=None)
    assert rc == INVALID and b"program is NULL" in msg and (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)
    for n in (0, 4096):
        rc, msg = extract(n=n)
        assert rc == INVALID and b"outside [1, 1024]" in msg, (n, msg)
    rc, msg = extract(algorithm=3)
    assert rc == INVALID and b"Unsupported algorithm" in msg
    for flags in (2, 0x80000000, 3):
        rc, msg = extract(flags=flags)
        assert rc == INVALID and b"unknown flags" in msg, (flags, msg)
    for a, b in ((None, hi), (lo, None)):
        rc, msg = extract(lo=a, hi=b)
        assert rc == INVALID and b"both" in msg, msg
    assert lib.sdfv_program_normal_points(None, 16, 1, 0.0, 16, None) == INVALID and b"program is NULL" in lib.sdfv_last_error()
    assert lib.sdfv_program_normal_points(prog.h, None, 1, 0.0, 16, None) == INVALID and b"NULL buffer" in lib.sdfv_last_error()
    assert lib.sdfv_program_normal_points(prog.h, 18, 1, 0.0, 16, None) == INVALID and b"4-byte aligned" in lib.sdfv_last_error()
    assert lib.sdfv_program_mesh_postproc(None, 16, 1, None) == INVALID and b"program is NULL" in lib.sdfv_last_error()
    assert lib.sdfv_program_mesh_postproc(prog.h, None, 1, None) == INVALID and b"NULL buffer" in lib.sdfv_last_error()
    assert lib.sdfv_program_mesh_postproc(prog.h, 18, 1, None) == INVALID and b"4-byte aligned" in lib.sdfv_last_error()
    assert lib.sdfv_program_mesh_postproc_host(None, 16, 1) == INVALID and b"program is NULL" in lib.sdfv_last_error()
    assert lib.sdfv_program_mesh_postproc_host(prog.h, None, 1) == INVALID and b"NULL buffer" in lib.sdfv_last_error()
    if lib.sdfv_device_count() == 0:
        for lo_, hi_ in ((lo, hi), (None, None)):
            rc, msg = extract(lo=lo_, hi=hi_)
            assert rc == NO_DEVICE and b"no HIP device" in msg
            assert (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)
        v = np.full((5, 12), 7.0, np.float32)
        assert lib.sdfv_program_mesh_postproc_host(prog.h, v.ctypes.data, 5) == NO_DEVICE and b"no HIP device" in lib.sdfv_last_error()
        assert (v == 7.0).all()
        assert lib.sdfv_program_mesh_postproc(prog.h, 16, 5, None) == NO_DEVICE
        assert lib.sdfv_program_normal_points(prog.h, 16, 5, 0.0, 16, None) == NO_DEVICE
    assert lib.sdfv_abi_version() == 5     # additive: the version stays


# ---- the built kernels (tests/kernel_objects.py) ----
INTERPRETING = ("sdfprog_mesh_lattice", "sdfprog_mesh_vertices", "sdfprog_mesh_vertices_mat", "sdfprog_mesh_postproc",
                "sdfprog_mesh_postproc_unaligned", "sdfprog_normal_points", "sdfprog_normal_points_staged")
POSITIONS = "mesh_edge_positions"                         # SDF-free and shared with the demo tree (mesh_kernels.hip)


def test_mesh_kernels_keep_the_resource_ceilings(code_objects):
    """DESIGN.md 3.7's ceilings for every sdfprog_mesh_* / sdfprog_normal_points* kernel and the positions kernel that runs
    between them, read from the built library: at most
    80 VGPRs (6 waves per SIMD), no scratch, no spill, at most 256 bytes of kernel arguments, and no vector memory operation
    inside an interpreter loop (the instruction fetch is scalar)."""
    table = kernel_table(code_objects)
    names = sorted(n for n in table if n.startswith(("sdfprog_mesh_", "sdfprog_normal_points")))
    assert set(names) == set(INTERPRETING), names
    assert POSITIONS in table
    names.append(POSITIONS)
    for name in names:
        k = table[name]
        assert k["vgpr"] <= 80, (name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k["kernarg"] <= 256, (name, k)
        ins = []                                          # [(opcode, address, branch target or None)]
        for ln in disassembly(k["co"], name).split("\n"):
            m = re.match(r"\s+(\S+)[^/]*//\s*([0-9A-Fa-f]{12}):[^<]*(?:<[^>+]*\+0x([0-9a-f]+)>)?", ln)
            if m:
                ins.append((m.group(1), int(m.group(2), 16), None if m.group(3) is None else int(m.group(3), 16)))
        ops = [i[0] for i in ins]
        assert not any(o.startswith(("scratch_", "buffer_")) for o in ops), name
        base = ins[0][1]
        back = [(base + to, at) for o, at, to in ins if o.startswith(("s_cbranch", "s_branch")) and to is not None and base + to < at]
        # an interpreter loop: a backward branch whose span holds the eighteen instruction bodies and a wide scalar load
        loops = []
        for lo, hi in back:
            body = [o for o, at, _ in ins if lo <= at <= hi]
            if len(body) > 200 and any(re.match(r"s_load_dwordx(4|8|16)$", o) for o in body):
                loops.append(body)
        if name not in INTERPRETING:
            assert not loops, name                        # the position kernel evaluates no SDF
            continue
        assert loops, (name, "no interpreter loop found")
        # the innermost such loop is the interpreter itself; the tap loop around it may load nothing per lane either
        inner = min(loops, key=len)
        assert not any(o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_")) for o in inner), name
    # the 48-byte record leaves as three 16-byte stores
    for name in ("sdfprog_mesh_vertices", "sdfprog_mesh_vertices_mat", "sdfprog_mesh_postproc"):
        ops = [ln.split("//")[0].split()[0] for ln in disassembly(table[name]["co"], name).split("\n") if ln.split("//")[0].split()]
        stores = [o for o in ops if o.startswith("global_store")]
        assert stores == ["global_store_dwordx4"] * 3, (name, stores)
    # the lattice pass: distance only -- one dword out, nothing in
    ops = [ln.split("//")[0].split()[0] for ln in disassembly(table["sdfprog_mesh_lattice"]["co"], "sdfprog_mesh_lattice").split("\n")
           if ln.split("//")[0].split()]
    assert [o for o in ops if o.startswith(("global_", "flat_"))] == ["global_store_dword"], ops


# ---- the restatement's own sanity: it is the yardstick of tests/test_gpu_program_mesh.py ----
@pytest.mark.parametrize("n", [16, 33])
def test_the_restated_sphere_is_a_closed_oriented_genus_0_surface(PM, n):
    b = R.catalogue(PM)["single"]
    v, idx, _ = M.extract(b.ops, n, b.bb)
    MR.assert_sphere_properties(v, idx, n)
    assert np.isfinite(v).all() and (v[:, 6:] == 0).all()


def test_the_restated_normal_and_postproc_follow_the_header(PM):
    """A sphere's default normal is radial to within the stencil's error; postproc keeps set normals bit for bit, recomputes
    unset ones, and takes raw material fields.  The bound: the four tetrahedral taps give 4e * grad + 4e^2 * (H_yz, H_xz, H_xy)
    + O(e^3), and a sphere's Hessian off the diagonal is -n_i n_j / r, at most 0.5 / r: a relative error of e * 0.5 / r, doubled
    for the normalisation.  Rounding: four distances of magnitude < 1 carry 4 * 2^-24 together, against a sum of 4e / sqrt(3)
    at the least -- 1e-4 at e = 0.001."""
    cat = R.catalogue(PM)
    pts = np.array([(0.6, 0, 0), (0, -0.6, 0), (0.3, 0.4, 0.5), (-0.2, 0.1, 0.9)], np.float32)
    n = M.normals(cat["single"].ops, pts)
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    r = np.linalg.norm(pts, axis=1, keepdims=True)
    assert (np.abs(n - radial) < 0.001 / r + 1e-4).all()
    assert (np.abs(M.normals(cat["single"].ops, pts, 0.01) - radial) < 0.01 / r + 1e-5).all()
    v = np.zeros((4, 12), np.float32)
    v[:, :3] = pts
    v[0, 3:6] = (0.0, 0.02, 0.0)                      # |n|^2 = 4e-4: kept
    v[1, 3:6] = (0.0, 0.009, 0.0)                     # 8.1e-5: recomputed
    v[2, 3:6] = (1.0, 2.0, 3.0)
    out = M.postproc(cat["all_ops"].ops, v)
    assert (M.bits(out[[0, 2], 3:6]) == M.bits(v[[0, 2], 3:6])).all()
    assert (M.bits(out[[1, 3], 3:6]) == M.bits(M.normals(cat["all_ops"].ops, pts[[1, 3]]))).all()
    assert (M.bits(out[:, 6:]) == M.bits(R.run(cat["all_ops"].ops, pts, False)[:, 1:])).all()
