"""Dual contouring on the device (include/sdfgrid.h, "Dual contouring"; algorithm 4) against the numpy restatement of
tests/mesh_ref.py (through tests/program_mesh_ref.py and tests/demo_mesh_ref.py), bit for bit, for SDF programs and for the demo tree: positions, normals, materials, indices; a
program whose gradient vanishes on its surface, an empty surface, a box that cuts the surface, the fused materials, the shared
scratch, the C++ host and the CLI."""
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import demo_mesh_ref as DM
import mesh_ref as MR
import program_mesh_ref as M
import program_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DUAL = MR.DUAL
UNIT_BOX = ((-1, -1, -1), (1, 1, 1))


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def cat(PM):
    return R.catalogue(PM)


@pytest.fixture(scope="module")
def built(cat):
    progs = {}

    def get(name):
        if name not in progs:
            progs[name] = cat[name].build()
        return progs[name]
    return get


@functools.lru_cache(maxsize=None)
def _restated(name, n, materials):
    PM = importlib.import_module("sdf-viewer_amd.program")
    b = R.catalogue(PM)[name]
    return M.extract(b.ops, n, b.bb, materials, DUAL)


def restated(name, n, materials=False):
    """The restatement's (vertices, indices, details) for a catalogue program: computed once, shared, never modified."""
    v, i, s = _restated(name, n, materials)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i, s


def arrays(v, i):
    return v.cpu().numpy(), i.cpu().numpy().astype(np.int64)


def assert_same_numbers(got, want, what):
    """Bit for bit where the restatement has a number; a NaN (unspecified payload and sign) where it has a NaN."""
    number = ~np.isnan(want)
    assert (M.bits(got)[number] == M.bits(want)[number]).all(), what
    assert np.isnan(got[~number]).all(), what


def assert_mesh_equal(got_v, got_i, want_v, want_i, what):
    assert got_v.shape == want_v.shape and got_i.shape == want_i.shape, (what, got_v.shape, want_v.shape, got_i.shape, want_i.shape)
    assert np.isfinite(want_v[:, :3]).all(), (what, "every restated position is finite")
    assert (M.bits(got_v[:, :3]) == M.bits(want_v[:, :3])).all(), (what, "positions")
    assert (got_i == want_i).all(), (what, "indices")
    assert_same_numbers(got_v[:, 3:6], want_v[:, 3:6], (what, "normals"))
    assert (M.bits(got_v[:, 6:]) == M.bits(want_v[:, 6:])).all(), (what, "material fields")


# (vertices, quads) the restatement gives (checked on the CPU); the three zeros are the empty-mesh cases
COUNTS = {("single", 5): (26, 24), ("anchor", 5): (0, 0), ("no_material", 5): (0, 0), ("all_ops", 5): (0, 0), ("deep", 5): (28, 26),
          ("ties", 5): (36, 30),
          ("single", 9): (146, 144), ("anchor", 9): (352, 360), ("no_material", 9): (80, 80), ("all_ops", 9): (18, 16),
          ("deep", 9): (93, 91), ("ties", 9): (74, 68),
          ("single", 12): (224, 222), ("anchor", 12): (832, 840), ("no_material", 12): (128, 128), ("all_ops", 12): (48, 46),
          ("deep", 12): (170, 169), ("ties", 12): (168, 162),
          # 65 cells: a row of 66 points spans two waves, 275 k cells, and the counts leave partial last workgroups
          ("anchor", 65): (34768, 34776)}


@pytest.mark.parametrize("name,n", sorted(COUNTS))
def test_programs_are_the_restatement_bit_for_bit(built, name, n):
    want_v, want_i, s = restated(name, n)
    assert (want_v.shape[0], s["quads"]) == COUNTS[(name, n)]          # so no comparison below passes vacuously
    v, i = built(name).mesh(n, algorithm=DUAL)
    if COUNTS[(name, n)][0] == 0:
        assert tuple(v.shape) == (0, 12) and tuple(i.shape) == (0,)
        return
    got_v, got_i = arrays(v, i)
    assert got_i.shape[0] == 6 * s["quads"]
    assert_mesh_equal(got_v, got_i, want_v, want_i, (name, n))
    assert (got_v[:, 6:] == 0).all()                                  # Vertex::default() without the flag


@pytest.mark.parametrize("kw,n,box,sdf_id,count", [
    (dict(), 9, UNIT_BOX, 0, (352, 360)),
    (dict(), 24, UNIT_BOX, 0, (4528, 4536)),
    (dict(), 12, UNIT_BOX, 1, (728, 726)),                            # the cube child on its own
])
def test_the_demo_tree_is_the_restatement_bit_for_bit(pkg, oracle, kw, n, box, sdf_id, count):
    prm = pkg.default_params(**kw)
    want_v, want_i, s = DM.extract_demo(oracle, oracle.params_from(prm), n, box, sdf_id, DUAL)
    assert (want_v.shape[0], s["quads"]) == count
    got_v, got_i = arrays(*pkg.mesh_extract(prm, n, *box, sdf_id=sdf_id, algorithm=DUAL))
    assert_mesh_equal(got_v, got_i, want_v, want_i, ("demo", n, sdf_id))
    assert (got_v[:, 6:] == 0).all()


def test_a_gradient_that_vanishes_on_the_surface(PM):
    """sphere(0.8) minus the plane x = 0 folded by SHELL 0: inside the sphere the distance is -|x|, which is -0 -- not inside -- on
    the lattice plane x = 0 (8 cells) and negative on both sides of it.  Every crossing edge there ends ON the plane, where the
    four taps of the normal are equal: the Hermite normal is NaN, the edge is not used, and a cell with k == 0 keeps its mass
    point.  The call returns, positions and indices equal the restatement."""
    b = PM.Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)).sphere(0.8).plane(1.0, 0.0, 0.0, 0.0).shell(0.0).subtract()
    n = 8
    _, d = M.lattice(b.ops, n, b.bb)
    hp = MR.edge_positions(d, b.bb)
    h = np.zeros((len(hp), 6), F)
    h[:, :3] = hp
    h[:, 3:6] = M.normals(b.ops, hp)
    s = MR.solve(d, b.bb, h)
    unsolved = s["used"] == 0
    assert np.isnan(h[:, 3:6]).any() and unsolved.sum() == 32 and (s["used"] < s["edges"]).sum() == 88 and len(s["pos"]) == 240
    assert np.isfinite(s["pos"]).all() and (M.bits(s["pos"][unsolved]) == M.bits(s["mass"][unsolved])).all()
    got_v, got_i = arrays(*b.build().mesh(n, algorithm=DUAL))
    assert got_v.shape[0] == 240 and (M.bits(got_v[:, :3]) == M.bits(s["pos"])).all()
    assert (got_i == s["idx"]).all()
    assert (M.bits(got_v[unsolved, :3]) == M.bits(s["mass"][unsolved])).all()


def test_an_empty_surface_gives_empty_arrays(pkg, PM):
    v, i = pkg.mesh_extract(pkg.default_params(sphere_radius=5.0), 8, sdf_id=2, algorithm=DUAL)   # everything inside
    assert tuple(v.shape) == (0, 12) and tuple(i.shape) == (0,)
    v, i = PM.Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)).sphere(5.0).build().mesh(8, algorithm=DUAL)
    assert tuple(v.shape) == (0, 12) and tuple(i.shape) == (0,)


def test_a_box_that_cuts_the_surface_leaves_it_open_there(pkg, oracle):
    """The demo in a box that ends at x = 0.5: crossing edges on the box's boundary emit nothing, so the triangle count is twice
    the INTERIOR crossing edges (fewer than the Hermite records), and every index is a vertex."""
    prm = pkg.default_params()
    box = ((-1, -1, -1), (0.5, 1, 1))
    want_v, want_i, s = DM.extract_demo(oracle, oracle.params_from(prm), 16, box, algorithm=DUAL)
    assert (want_v.shape[0], s["quads"], len(s["hermite"])) == (1436, 1400, 1480)
    got_v, got_i = arrays(*pkg.mesh_extract(prm, 16, *box, algorithm=DUAL))
    assert got_i.shape[0] == 3 * 2 * s["quads"] and got_i.min() >= 0 and got_i.max() < got_v.shape[0]
    assert_mesh_equal(got_v, got_i, want_v, want_i, "cut box")


@pytest.mark.parametrize("name,n", [("all_ops", 12), ("deep", 12), ("ties", 9)])
def test_fused_materials_equal_extract_then_postproc_and_the_restatement(built, name, n):
    want_v, want_i, _ = restated(name, n, True)
    assert want_v.shape[0] > 0 and np.isfinite(want_v).all()
    prog = built(name)
    fv, fi = prog.mesh(n, materials=True, algorithm=DUAL)
    pv, pi = prog.mesh(n, algorithm=DUAL)
    assert (pv[:, 6:] == 0).all()
    prog.mesh_postproc(pv)
    torch.cuda.synchronize()
    assert_mesh_equal(*arrays(fv, fi), want_v, want_i, (name, n, "fused"))
    assert_mesh_equal(*arrays(pv, pi), want_v, want_i, (name, n, "extract + postproc"))
    assert (M.bits(fv.cpu().numpy()) == M.bits(pv.cpu().numpy())).all()


def test_marching_cubes_and_dual_contouring_share_the_scratch(pkg, built):
    prm = pkg.default_params()

    def both(algorithm):
        dv, di = pkg.mesh_extract(prm, 24, algorithm=algorithm)
        pv, pi = built("deep").mesh(12, algorithm=algorithm)
        return [x.cpu().numpy() for x in (dv, di, pv, pi)]
    first = both(0)
    dual = both(DUAL)
    again = both(0)
    for a, b in zip(first, again):
        assert a.shape[0] > 0 and a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()
    assert dual[0].shape[0] == 4528 and dual[2].shape[0] == 170
    assert pkg.lib.sdfv_mesh_trim() == 0
    for a, b in zip(dual, both(DUAL)):
        assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def test_cpp_host_and_cli_mesh_with_dual_contouring(pkg, host, built, cat, tmp_path):
    """tests/c/dual_contour_host.cpp (ProgramSDF -> mesh_sdf -> postproc -> PLY), host.Mesh.from_sdf over the demo, and
    `sdf-viewer-gpu mesh ... dual-contouring-particle-based-minimization demo`: the library's arrays and counts."""
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "dual_contour_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(lib, "host"),
                           os.path.join(ROOT, "tests", "c", "dual_contour_host.cpp"), "-o", str(exe), "-L", lib, "-lsdfviewer_host",
                           "-lsdfgrid", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                           "-Wl,-rpath," + lib, "-ldl", "-pthread"])
    b = cat["deep"]
    assert tuple(b.bb) == (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)            # the driver's box
    ops_file = tmp_path / "ops.bin"
    ops_file.write_bytes(bytes(b.array())[:64 * len(b.ops)])
    n = 12
    r = subprocess.run([str(exe), str(ops_file), str(n), str(tmp_path / "v.bin"), str(tmp_path / "i.bin"), str(tmp_path / "m.ply")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dual_contour_host ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    got_v = np.fromfile(tmp_path / "v.bin", F).reshape(-1, 12)
    got_i = np.fromfile(tmp_path / "i.bin", np.uint32).astype(np.int64)
    pv, pi = (x.cpu().numpy() for x in built("deep").mesh(n, materials=True, algorithm=DUAL))
    assert pv.shape[0] == 170
    assert_mesh_equal(got_v, got_i, pv, pi.astype(np.int64), "C++ host against the Python route")
    ply = (tmp_path / "m.ply").read_text().split("\n")
    assert ply[0] == "ply" and f"element vertex {pv.shape[0]}" in ply and f"element face {pi.shape[0] // 3}" in ply
    # the demo through the host library
    prm = pkg.default_params(sphere_radius=0.9)
    name = "dual-contouring-particle-based-minimization"
    hv, hi = host.Mesh.from_sdf(host.SDF.demo("-s", "0.9"), mesher=name, max_voxels_per_axis=20, postproc=False).arrays()
    dv, di = (x.cpu().numpy() for x in pkg.mesh_extract(prm, 20, algorithm=DUAL))
    assert dv.shape[0] > 0 and (M.bits(hv) == M.bits(dv)).all() and (hi.astype(np.int64) == di.astype(np.int64)).all()
    # ... and the CLI
    out = tmp_path / "cli.ply"
    cli = os.path.join(lib, "sdf-viewer-gpu")
    r = subprocess.run([cli, "mesh", "-o", str(out), "-v", "20", name, "demo", "-s", "0.9"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    text = out.read_text().split("\n")
    assert f"element vertex {dv.shape[0]}" in text and f"element face {di.shape[0] // 3}" in text
    body = text[text.index("end_header") + 1:]
    xyz = np.array([[float(x) for x in ln.split()[:3]] for ln in body[:dv.shape[0]]], np.float64).astype(F)
    assert (xyz == dv[:, :3]).all()
    faces = np.array([[int(x) for x in ln.split()] for ln in body[dv.shape[0]:dv.shape[0] + di.shape[0] // 3]], np.int64)
    assert (faces[:, 0] == 3).all() and (faces[:, 1:].reshape(-1) == di.astype(np.int64)).all()
