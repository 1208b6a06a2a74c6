"""CPU tests of meshing a sampled lattice (include/sdfgrid.h, "Meshing a sampled lattice"): the sanity of the numpy restatement
the GPU tests compare against (tests/lattice_mesh_ref.py over tests/mesh_ref.py) on geometry whose answer is known (its bits are
pinned by tests/test_mesh_ref_pins.py); what the four entry points refuse without a device, with code and text; and what the built kernels look
like.  No device needed."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import lattice_mesh_ref as L
import mesh_ref as MR
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

INVALID, NO_DEVICE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
F = np.float32


# ---- the restatement: it is the yardstick of tests/test_gpu_lattice_mesh.py ----
def fibonacci_sphere(m):
    i = np.arange(m) + 0.5
    phi, theta = np.arccos(1.0 - 2.0 * i / m), np.pi * (1.0 + 5.0 ** 0.5) * i
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=-1)


@pytest.mark.parametrize("n,degrees", [(5, 1.71), (12, 0.98), (24, 0.23)])
def test_the_restated_normal_reproduces_the_header_s_sphere_table(n, degrees):
    """A sphere of radius 0.6 in [-1, 1]^3, its exact distance at the lattice points, 4000 points on the surface: the worst angle
    between the restated normal and the true one is the figure the header quotes, within 5 % of it."""
    u = fibonacci_sphere(4000)
    got = MR.lattice_normals(L.sphere_lattice(n, BOX), BOX, (u * 0.6).astype(F)).astype(np.float64)
    assert (np.abs(np.linalg.norm(got, axis=1) - 1.0) < 1e-6).all()
    worst = np.degrees(np.arccos(np.clip((got * u).sum(axis=1), -1.0, 1.0))).max()
    print(n, "cells: worst angle to the true normal", worst, "degrees; the header says", degrees)
    assert abs(worst - degrees) <= 0.05 * degrees


def test_the_restated_normal_is_exact_on_a_linear_field_clamps_outside_and_is_zero_where_the_gradient_is():
    """d = a . p + b: every difference quotient is the gradient itself, so the normal is a / |a| to rounding anywhere, outside
    the box included (the clamp takes the border cell).  A constant lattice has no gradient: the zero normal."""
    n, bb = 7, (-1.0, -0.5, 0.0, 1.0, 1.5, 3.0)
    a = np.array([0.3, -0.5, 0.8])
    d = (MR.lattice_points(n, bb).astype(np.float64) @ a + 0.05).astype(F).reshape(n + 1, n + 1, n + 1)
    pts = np.array([(0.1, 0.2, 0.3), (-1.0, -0.5, 0.0), (1.0, 1.5, 3.0), (5.0, -7.0, 1.0), (0.999, 1.499, 2.999)], F)
    got = MR.lattice_normals(d, bb, pts)
    assert np.abs(got - (a / np.linalg.norm(a))[None, :]).max() < 1e-5
    flat = np.full((n + 1, n + 1, n + 1), 0.25, F)
    assert (L.bits(MR.lattice_normals(flat, bb, pts)) == 0).all()


@pytest.mark.parametrize("n", [9, 12])
def test_the_restated_sphere_is_a_closed_oriented_genus_0_surface(n):
    v, i, _ = L.extract(L.sphere_lattice(n, BOX), BOX)
    MR.assert_sphere_properties(v, i, n)


# ---- the ABI ----
def test_every_new_entry_point_is_declared_exported_and_bound(pkg):
    names = ("sdfv_lattice_points", "sdfv_lattice_from_samples", "sdfv_lattice_mesh_extract", "sdfv_lattice_normals")
    header = open(os.path.join(ROOT, "include", "sdfgrid.h")).read()
    raw = C.CDLL(pkg._capi.LIB_PATH)
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in pkg._capi.PROTOTYPES and getattr(raw, name)
    assert "Meshing a sampled lattice" in header
    for name in ("lattice_points", "lattice_from_samples", "lattice_mesh_extract", "lattice_normals", "mesh_extract"):
        assert callable(getattr(pkg, name)), name
    assert pkg.lib.sdfv_abi_version() == 5     # additive: the version stays


def test_argument_errors_come_first_and_without_a_device_nothing_is_written(pkg):
    lib, K = pkg.lib, pkg._capi
    lo, hi = pkg.f3((-1, -1, -1)), pkg.f3((1, 1, 1))
    m = K.Mesh()
    dist = 4096                                           # any non-NULL, 4-byte aligned address: nothing reads it before the device check

    def extract(dist=dist, lo=lo, hi=hi, n=8, algorithm=0, flags=0, out=m):
        m.vertices, m.indices, m.n_vertices, m.n_indices = 1, 1, 7, 7
        rc = lib.sdfv_lattice_mesh_extract(dist, lo, hi, n, algorithm, flags, None if out is None else C.byref(out), None)
        return rc, lib.sdfv_last_error()

    def cleared():
        return (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)

    assert extract(out=None) == (INVALID, b"out is NULL")
    assert extract(dist=None) == (INVALID, b"dist is NULL") and cleared()
    for a, b in ((None, hi), (lo, None), (None, None)):
        assert extract(lo=a, hi=b) == (INVALID, b"bounding box is NULL") and cleared()
    rc, msg = extract(dist=4098)
    assert rc == INVALID and b"4-byte aligned" in msg
    for algorithm in (1, 2, 3, 5):
        assert extract(algorithm=algorithm) == (INVALID, b"Unsupported algorithm %d" % algorithm) and cleared()
    for n in (0, 1025, 4096):
        rc, msg = extract(n=n)
        assert rc == INVALID and msg == b"max_voxels_per_axis %d is outside [1, 1024]" % n, (n, msg)
    for flags in (1, 2, 0x80000000):
        assert extract(flags=flags) == (INVALID, b"unknown flags 0x%x" % flags)

    def normals(dist=dist, lo=lo, hi=hi, cells=8, vertices=4096, n=5):
        return lib.sdfv_lattice_normals(dist, lo, hi, cells, vertices, n, None), lib.sdfv_last_error()

    assert normals(dist=None) == (INVALID, b"dist is NULL")
    assert normals(lo=None) == (INVALID, b"bounding box is NULL")
    assert normals(hi=None) == (INVALID, b"bounding box is NULL")
    for cells in (0, 1025):
        rc, msg = normals(cells=cells)
        assert rc == INVALID and b"outside [1, 1024]" in msg
    assert normals(vertices=None) == (INVALID, b"NULL buffer")
    rc, msg = normals(vertices=4098)
    assert rc == INVALID and b"4-byte aligned" in msg

    def points(lo=lo, hi=hi, cells=8, first=0, n=729, out=4096):
        return lib.sdfv_lattice_points(lo, hi, cells, first, n, out, None), lib.sdfv_last_error()

    assert points(lo=None) == (INVALID, b"bounding box is NULL")
    for cells in (0, 1025):
        rc, msg = points(cells=cells)
        assert rc == INVALID and b"outside [1, 1024]" in msg
    for first, n in ((0, 730), (729, 1), (730, 0), (2 ** 40, 1), (1, 2 ** 64 - 1)):
        rc, msg = points(first=first, n=n)
        assert rc == INVALID and b"not all among the lattice's 729" in msg, (first, n, msg)
    assert points(out=None) == (INVALID, b"NULL buffer")
    assert lib.sdfv_lattice_from_samples(None, 3, 4096, None) == INVALID and lib.sdfv_last_error() == b"NULL buffer"
    assert lib.sdfv_lattice_from_samples(4096, 3, None, None) == INVALID and lib.sdfv_last_error() == b"NULL buffer"
    assert lib.sdfv_lattice_from_samples(4098, 3, 4096, None) == INVALID and b"4-byte aligned" in lib.sdfv_last_error()
    if lib.sdfv_device_count() == 0:
        for algorithm in (0, 4):
            rc, msg = extract(algorithm=algorithm)
            assert rc == NO_DEVICE and b"no HIP device" in msg and cleared()
        v = np.full((5, 12), 7.0, F)
        assert normals(vertices=v.ctypes.data)[0] == NO_DEVICE and (v == 7.0).all()
        assert points()[0] == NO_DEVICE
        assert lib.sdfv_lattice_from_samples(4096, 3, 4096, None) == NO_DEVICE
    # empty requests need no buffer
    assert normals(vertices=None, n=0)[0] in (0, NO_DEVICE)
    assert points(n=0, out=None, first=729)[0] in (0, NO_DEVICE)


# ---- the built kernels (tests/kernel_objects.py) ----
KERNELS = ("lattice_points", "lattice_from_samples", "lattice_normals", "lattice_normals_zero_mat")


def stream_of(k, name):
    return [ln.split("//")[0].split()[0] for ln in disassembly(k["co"], name).split("\n") if ln.split("//")[0].split()]


def dwords(op):
    m = re.search(r"dwordx(\d)", op)
    return int(m.group(1)) if m else 1


def test_lattice_kernels_keep_the_resource_ceilings(code_objects):
    """no scratch, no spill, no LDS, at most 64 VGPRs -- the 8-waves-per-SIMD step the dual-contour kernels hold
    (59 were read for the two normal kernels).  The normal kernel's corner loop is a loop: a backward branch around 12 loads, not
    48 loads in a row; what it stores is the three dwords of the normal and nothing else (the _zero_mat form: the six material
    dwords too); nothing is contracted."""
    table = kernel_table(code_objects)
    assert sorted(n for n in table if n.startswith("lattice_")) == sorted(KERNELS)
    for name in KERNELS:
        k = table[name]
        print(name, {a: b for a, b in k.items() if a != "co"})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] <= 64, (name, k)
        assert k["kernarg"] <= 256, (name, k)
        ops = stream_of(k, name)
        assert not any(o.startswith(("scratch_", "buffer_", "ds_", "flat_")) for o in ops), name
        assert not any(o.startswith("v_pk_fma") for o in ops), name
    for name, stored in (("lattice_normals", 3), ("lattice_normals_zero_mat", 9)):
        k = table[name]
        ops = stream_of(k, name)
        assert sum(dwords(o) for o in ops if o.startswith("global_store")) == stored, (name, ops)
        loads = [o for o in ops if o.startswith("global_load")]
        assert sum(dwords(o) for o in loads) == 3 + 12, (name, loads)  # the position, then one round of the corner loop
        ins = []
        for ln in disassembly(k["co"], name).split("\n"):
            mm = re.match(r"\s+(\S+)[^/]*//\s*([0-9A-Fa-f]{12}):[^<]*(?:<[^>+]*\+0x([0-9a-f]+)>)?", ln)
            if mm:
                ins.append((mm.group(1), int(mm.group(2), 16), None if mm.group(3) is None else int(mm.group(3), 16)))
        base = ins[0][1]
        back = [(base + to, at) for o, at, to in ins if o.startswith(("s_cbranch", "s_branch")) and to is not None and base + to < at]
        assert back, (name, "no loop")
        assert any(sum(dwords(o) for o, at, _ in ins if lo <= at <= hi and o.startswith("global_load")) == 12 for lo, hi in back), name
    assert [o for o in stream_of(table["lattice_from_samples"], "lattice_from_samples") if o.startswith("global_")] == \
        ["global_load_dword", "global_store_dword"]
    assert sum(dwords(o) for o in stream_of(table["lattice_points"], "lattice_points") if o.startswith("global_")) == 3
