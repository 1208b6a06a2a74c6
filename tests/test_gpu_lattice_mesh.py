"""Meshing a sampled lattice on the device (include/sdfgrid.h, "Meshing a sampled lattice") against the numpy restatement of
tests/lattice_mesh_ref.py (over tests/mesh_ref.py), bit for bit in positions, normals and indices, under marching cubes and dual contouring: lattices from
programs, a gyroid that cuts the box, seeded noise that reaches all 256 cube cases, a box that is no cube, an empty mesh, zero
gradients; the three helper entry points; the one scratch pool; the C++ host route and the command line."""
import ctypes as C
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import lattice_mesh_ref as L
import mesh_ref as MR
import program_mesh_ref as M
import program_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
SLAB_BOX = (-1.0, -0.5, -0.75, 1.0, 0.5, 0.75)              # no cube: three different cell sides
SPHERE = ((R.SPHERE, (0.6,)),)
CUBE_MINUS_SPHERE = ((R.CUBE, (0.61,)), (R.SPHERE, (0.72,)), (R.SUBTRACT, ()))   # no lattice point of 5, 9 or 12 cells on a face
ALGORITHMS = (0, L.DUAL)


def noise(n, seed=0):
    """Independent values in +-[0.1, 1]: nothing like a distance field, every cube case (12 cells, seed 0: all 256)."""
    r = np.random.default_rng(seed)
    shape = (n + 1, n + 1, n + 1)
    return (r.uniform(0.1, 1.0, shape) * np.where(r.random(shape) < 0.5, -1.0, 1.0)).astype(F)


def alternating(n):
    """+-0.5 alternating along x, constant along y and z: every x edge crosses, and the central difference of every interior
    point is exactly zero -- the interior vertices' gradient has s = 0, the border columns' (one-sided) has not."""
    row = np.where(np.arange(n + 1) % 2 == 0, F(0.5), F(-0.5))
    return np.broadcast_to(row, (n + 1, n + 1, n + 1)).copy()


@functools.lru_cache(maxsize=None)
def lattice(kind, n):
    """(d [k, j, i] float32, bb) of a named test lattice: computed once, shared, never modified."""
    if kind == "sphere":
        d, bb = M.lattice(SPHERE, n, BOX)[1], BOX
    elif kind == "cube-sphere":
        d, bb = M.lattice(CUBE_MINUS_SPHERE, n, BOX)[1], BOX
    elif kind == "gyroid":
        d, bb = L.gyroid_lattice(n, BOX), BOX
    elif kind == "gyroid-slab":
        d, bb = L.gyroid_lattice(n, SLAB_BOX), SLAB_BOX
    elif kind == "noise":
        d, bb = noise(n), BOX
    elif kind == "alternating":
        d, bb = alternating(n), BOX
    else:
        d, bb = np.full((n + 1, n + 1, n + 1), 0.25, F), BOX                      # "positive": nothing to mesh
    d = np.ascontiguousarray(d, F)
    d.setflags(write=False)
    return d, bb


@functools.lru_cache(maxsize=None)
def restated(kind, n, algorithm):
    d, bb = lattice(kind, n)
    v, i, info = L.extract(d, bb, algorithm)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i, info


def to_dev(d):
    return torch.from_numpy(np.array(d, F)).cuda()                     # (a copy: the shared lattices are read-only)


def host(v, i):
    return v.cpu().numpy(), i.cpu().numpy().astype(np.int64)


def assert_mesh_equal(got_v, got_i, want_v, want_i, what):
    assert got_v.shape == want_v.shape and got_i.shape == want_i.shape, (what, got_v.shape, want_v.shape, got_i.shape, want_i.shape)
    assert (L.bits(got_v[:, :3]) == L.bits(want_v[:, :3])).all(), (what, "positions")
    assert (got_i == want_i).all(), (what, "indices")
    assert (L.bits(got_v[:, 3:6]) == L.bits(want_v[:, 3:6])).all(), (what, "normals")
    assert (L.bits(got_v[:, 6:]) == 0).all(), (what, "colour and material fields are 0")


# 65 cells: a row of 66 points spans two waves, 287 k points, and neither vertex count is a multiple of 64
CASES = [(kind, n) for kind in ("sphere", "cube-sphere", "gyroid", "gyroid-slab", "alternating") for n in (5, 9, 12)] + \
        [("noise", 12), ("gyroid-slab", 65)]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("kind,n", CASES)
def test_extraction_is_the_restatement_bit_for_bit(pkg, kind, n, algorithm):
    d, bb = lattice(kind, n)
    want_v, want_i, info = restated(kind, n, algorithm)
    assert want_v.shape[0] > 0 and want_i.shape[0] > 0 and np.isfinite(want_v).all()   # no comparison passes vacuously
    if kind == "noise" and algorithm == 0:
        assert len(np.unique(info["cases"])) == 256
    if kind.startswith("gyroid") and algorithm == 0:                   # the surface leaves the box: one-sided differences are used
        lo, hi = np.array(bb[:3], F), np.array(bb[3:], F)
        assert ((want_v[:, :3] == lo) | (want_v[:, :3] == hi)).any()
    zero_normals = (want_v[:, 3:6] == 0).all(axis=1)
    if kind == "alternating":
        assert zero_normals.any() and not zero_normals.all()
    else:
        assert not zero_normals.any()
    if n == 65:
        assert want_v.shape[0] % 64 != 0 and (algorithm == 0 or len(info["hermite"]) % 64 != 0)
    dev = to_dev(d)
    keep = dev.clone()
    v, i = pkg.lattice_mesh_extract(dev, bb, n, algorithm)
    assert torch.equal(dev, keep), "dist is read, never written"
    got_v, got_i = host(v, i)
    assert got_i.shape[0] % 3 == 0
    assert_mesh_equal(got_v, got_i, want_v, want_i, (kind, n, algorithm))


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_an_all_positive_lattice_gives_an_empty_mesh(pkg, algorithm):
    d, bb = lattice("positive", 9)
    v, i = pkg.lattice_mesh_extract(to_dev(d), bb, 9, algorithm)
    assert tuple(v.shape) == (0, 12) and tuple(i.shape) == (0,)


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("name,ops,n", [("sphere", SPHERE, 12), ("cube-sphere", CUBE_MINUS_SPHERE, 9), ("sphere", SPHERE, 65)])
def test_positions_and_indices_equal_the_program_s_own_extraction(pkg, PM, name, ops, n, algorithm):
    """The lattice of the program's distances (the restatement's, which the device's lattice pass equals bit for bit:
    tests/test_gpu_program_mesh.py) meshed by the lattice route against sdfv_program_mesh_extract on the same program."""
    builder = PM.Program(BOX)
    for opcode, operands in ops:
        builder.op(opcode, *operands)
    pv, pi = host(*builder.build().mesh(n, algorithm=algorithm))
    d = M.lattice(ops, n, BOX)[1]
    assert not (d == 0).any()
    gv, gi = host(*pkg.lattice_mesh_extract(torch.from_numpy(np.ascontiguousarray(d, F)).cuda(), BOX, n, algorithm))
    assert pv.shape[0] > 0 and gv.shape == pv.shape and gi.shape == pi.shape
    if algorithm == 0:                                                 # marching cubes: positions depend on the distances alone
        assert (L.bits(gv[:, :3]) == L.bits(pv[:, :3])).all()
    else:                                                              # dual contouring solves with each route's own normals
        assert np.abs(gv[:, :3] - pv[:, :3]).max() <= 2.0 / n
    assert (gi == pi).all()


def test_the_scratch_is_shared_with_program_extractions(pkg, PM):
    prog = PM.Program(BOX).sphere(0.6).build()

    def round_trip():
        out = []
        for step in (("program", 33, 0), ("gyroid", 12, 0), ("program", 5, 4), ("noise", 12, 4), ("gyroid-slab", 65, 4),
                     ("program", 12, 0), ("sphere", 5, 0)):
            if step[0] == "program":
                v, i = prog.mesh(step[1], algorithm=step[2])
            else:
                d, bb = lattice(step[0], step[1])
                v, i = pkg.lattice_mesh_extract(to_dev(d), bb, step[1], step[2])
            out.append(host(v, i))
        return out
    before = round_trip()
    for k, (kind, n, algorithm) in ((1, ("gyroid", 12, 0)), (3, ("noise", 12, 4)), (4, ("gyroid-slab", 65, 4)), (6, ("sphere", 5, 0))):
        want_v, want_i, _ = restated(kind, n, algorithm)
        assert_mesh_equal(before[k][0], before[k][1], want_v, want_i, (kind, n, algorithm))
    assert pkg.lib.sdfv_mesh_trim() == 0
    after = round_trip()
    for (bv, bi), (av, ai) in zip(before, after):
        assert bv.shape[0] > 0 and (L.bits(bv) == L.bits(av)).all() and (bi == ai).all()


def test_lattice_points_over_a_range_that_spans_a_row_end_and_a_plane_end(pkg):
    n, bb = 12, SLAB_BOX                                               # rows of 13, planes of 169
    want = MR.lattice_points(n, bb)
    for first, count in ((100, 300), (0, 13 ** 3), (13 ** 3 - 1, 1), (169, 0)):
        got = pkg.lattice_points(bb, n, first, count).cpu().numpy()
        assert got.shape == (count, 3) and (L.bits(got) == L.bits(want[first:first + count])).all(), (first, count)
    assert 100 % 64 != 0 and 100 // 13 != 399 // 13 and 100 // 169 != 399 // 169
    with pytest.raises(pkg.SdfvError):
        pkg.lattice_points(bb, n, 13 ** 3 - 1, 2)


def test_lattice_from_samples_takes_the_distances(pkg):
    rng = np.random.default_rng(3)
    s = rng.normal(size=(1000, 7)).astype(F)
    got = pkg.lattice_from_samples(torch.from_numpy(s).cuda()).cpu().numpy()
    assert (L.bits(got) == L.bits(s[:, 0])).all()


@pytest.mark.parametrize("kind,n", [("gyroid-slab", 9), ("noise", 12), ("alternating", 9)])
def test_lattice_normals_inside_cells_and_outside_the_box(pkg, kind, n):
    """Arbitrary points -- inside cells, on the box's faces and corners, outside the box on every side (the clamp) -- through a
    pointer that is only 4-byte aligned: the three floats of the normal equal the restatement, the other nine stay as they were."""
    d, bb = lattice(kind, n)
    lo, hi = np.array(bb[:3]), np.array(bb[3:])
    rng = np.random.default_rng(n)
    m = 1300
    p = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), size=(m, 3))
    p[:400] = rng.uniform(lo, hi, size=(400, 3))
    p[400:408] = [[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)]
    inside = ((p >= lo) & (p <= hi)).all(axis=1)
    assert inside.sum() > 400 and (~inside).sum() > 400
    v = np.full((m, 12), 9.0, F)
    v[:, :3] = p.astype(F)
    want = v.copy()
    want[:, 3:6] = MR.lattice_normals(d, bb, v[:, :3])
    assert np.isfinite(want).all()
    dev = to_dev(d)
    for offset in (0, 1):
        buf = torch.zeros(m * 12 + 4, dtype=torch.float32, device="cuda")
        t = buf[offset:offset + m * 12].view(m, 12)
        assert t.data_ptr() % 16 == 4 * offset
        t.copy_(torch.from_numpy(v))
        pkg.lattice_normals(dev, bb, n, t)
        got = t.cpu().numpy()
        assert (L.bits(got) == L.bits(want)).all(), offset
        assert (buf[:offset] == 0).all() and (buf[offset + m * 12:] == 0).all(), offset


# ---- the C++ host and the command line ----
def build_host(tmp_path):
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "lattice_mesh_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(lib, "host"),
                           os.path.join(ROOT, "tests", "c", "lattice_mesh_host.cpp"), "-o", str(exe), "-L", lib, "-lsdfviewer_host",
                           "-lsdfgrid", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                           "-Wl,-rpath," + lib, "-ldl", "-pthread"])
    return exe


def test_cpp_host_meshes_surfaces_without_a_device_form(tmp_path):
    """tests/c/lattice_mesh_host.cpp, linked against the product library: mesh_any_sdf over a host-only surface (4 threads) and
    over a device-sampled one equals the lattice calls made by hand, a throwing surface is an error, postproc_any is
    meshers/mesh.rs:22-33, mesh_sdf still refuses -- and the 12-cell meshes it leaves equal the restatement over its lattice."""
    exe = build_host(tmp_path)
    prefix = tmp_path / "host"
    r = subprocess.run([str(exe), str(prefix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lattice_mesh_host ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    n, bb = 12, (-1.0, -0.9, -0.8, 1.0, 0.9, 0.8)
    d = np.fromfile(str(prefix) + ".dist.bin", F).reshape(n + 1, n + 1, n + 1)
    for algorithm in ALGORITHMS:
        got_v = np.fromfile(f"{prefix}.v{algorithm}.bin", F).reshape(-1, 12)
        got_i = np.fromfile(f"{prefix}.i{algorithm}.bin", np.uint32).astype(np.int64)
        want_v, want_i, _ = L.extract(d, bb, algorithm)
        assert_mesh_equal(got_v, got_i, want_v, want_i, ("C++ host", algorithm))


def parse_ply(text):
    lines = text.split("\n")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    body = lines[lines.index("end_header") + 1:]
    verts = np.array([[float(x) for x in ln.split()] for ln in body[:nv]], np.float64).reshape(nv, 12)
    faces = np.array([[int(x) for x in ln.split()] for ln in body[nv:nv + nf]], np.int64).reshape(nf, 4)
    return verts, faces


def test_cli_meshes_a_provider_library(pkg, gyroid_provider, tmp_path):
    """`sdf-viewer-gpu mesh -v 12 -o out.ply url file://libgyroid_provider.so`: the PLY's vertices and faces are those of the C
    API over the lattice of the same provider's samples (its corner point is a NaN: not inside, like any other)."""
    exe = os.path.join(ROOT, "sdf-viewer_amd", "sdf-viewer-gpu")
    out = tmp_path / "gyroid.ply"
    r = subprocess.run([exe, "mesh", "-v", "12", "-o", str(out), "url", "file://" + gyroid_provider], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    verts, faces = parse_ply(open(out).read())
    n, bb = 12, (-1.0, -0.5, -0.75, 1.0, 0.5, 0.75)
    raw = C.CDLL(gyroid_provider)
    pts = MR.lattice_points(n, bb)
    d = np.zeros(len(pts), F)
    rec = np.zeros(7, F)
    for k, p in enumerate(pts):
        raw.gyroid_sample_raw(None, p.ctypes.data_as(C.c_void_p), 1, rec.ctypes.data_as(C.c_void_p))
        d[k] = rec[0]
    assert np.isnan(d).sum() == 1
    v, i = host(*pkg.lattice_mesh_extract(to_dev(d), bb, n))
    assert v.shape[0] > 100 and verts.shape[0] == v.shape[0] and faces.shape[0] * 3 == i.shape[0]
    np.testing.assert_array_equal(verts[:, :3].astype(F), v[:, :3])
    np.testing.assert_array_equal(faces[:, 1:].reshape(-1), i)
    r = subprocess.run([exe, "mesh", "url", "http://example.invalid/sdf.wasm"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "only local provider libraries" in r.stderr      # the URL rules of `app`


def test_cli_mesh_demo_is_still_mesh_sdf(host, tmp_path):
    """`sdf-viewer-gpu mesh ... demo` goes through mesh_any_sdf and postproc_any now: the same mesh as mesh_sdf + Mesh::postproc."""
    exe = os.path.join(ROOT, "sdf-viewer_amd", "sdf-viewer-gpu")
    out = tmp_path / "demo.ply"
    r = subprocess.run([exe, "mesh", "-o", str(out), "-v", "16", "demo", "-s", "0.9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    verts, faces = parse_ply(open(out).read())
    v, i = host.Mesh.from_sdf(host.SDF.demo("-s", "0.9"), max_voxels_per_axis=16).arrays()
    assert v.shape[0] > 0 and verts.shape[0] == v.shape[0]
    np.testing.assert_array_equal(verts[:, :6].astype(F), v[:, :6])
    np.testing.assert_array_equal(verts[:, 9:].astype(F), v[:, 9:])
    np.testing.assert_array_equal(faces[:, 1:].reshape(-1), i.astype(np.int64))
