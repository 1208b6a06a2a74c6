"""The device mesher (sdfv_mesh_extract): the extraction algorithm is the build's own (the reference delegates to the
un-vendored `isosurface` crate), so the checks are (1) the numpy restatement of the same conventions (tests/mesh_ref.py
through tests/demo_mesh_ref.py; tools/gen_mc_table.py documents them) fed with the ORACLE's lattice distances and normals --
vertices and indices must match exactly -- and (2) properties any correct extractor has: closed 2-manifold, outward orientation, Euler
characteristic, vertices on the surface."""
import os

import numpy as np
import pytest
import torch

import demo_mesh_ref as DM
import mesh_ref as MR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sdf_id,kw,box,n", [
    (2, dict(sphere_radius=0.8), ((-1, -1, -1), (1, 1, 1)), 12),
    (0, dict(), ((-1, -1, -1), (1, 1, 1)), 16),
    (1, dict(cube_half_side=0.6), ((-1.0, -0.75, -1.25), (1.0, 1.0, 0.5)), 9),
    (0, dict(cube_half_side=0.7, sphere_radius=0.8), ((-1, -1, -1), (1, 1, 1)), 11),
])
def test_extraction_matches_numpy_restatement(pkg, oracle, sdf_id, kw, box, n):
    prm = pkg.default_params(**kw)
    oprm = oracle.params_from(prm)
    v, idx = pkg.mesh_extract(prm, n, *box, sdf_id=sdf_id)
    want_v, want_i, _ = DM.extract_demo(oracle, oprm, n, box, sdf_id)
    assert v.shape[0] == want_v.shape[0] and idx.shape[0] == want_i.shape[0]
    got = v.cpu().numpy()
    np.testing.assert_array_equal(MR.bits(got[:, :3]), MR.bits(want_v[:, :3]))
    np.testing.assert_array_equal(idx.cpu().numpy().astype(np.int64), want_i)
    # normals = HermiteSource at the vertex (the oracle's normal_many), material fields = Vertex::default()
    np.testing.assert_array_equal(MR.bits(got[:, 3:6]), MR.bits(want_v[:, 3:6]))
    assert (got[:, 6:] == 0).all()


@pytest.mark.parametrize("n", [16, 33, 64])
def test_sphere_is_a_closed_oriented_genus_0_surface(pkg, oracle, n):
    prm = pkg.default_params(sphere_radius=0.8)
    v, idx = pkg.mesh_extract(prm, n, sdf_id=2)
    v, idx = v.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    n_edges = MR.manifold_edges(idx)
    assert v.shape[0] - n_edges + idx.shape[0] // 3 == 2  # Euler characteristic of a sphere
    assert idx.min() == 0 and idx.max() == v.shape[0] - 1 and len(np.unique(idx)) == v.shape[0]
    r = np.linalg.norm(v[:, :3].astype(np.float64), axis=1)
    assert np.abs(r - 0.8).max() < (2.0 / n) ** 2  # linear interpolation of an exact distance: O(h^2) off the sphere
    tri = v[idx.reshape(-1, 3), :3].astype(np.float64)
    face_n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    centroid = tri.mean(axis=1)
    assert (np.einsum("ij,ij->i", face_n, centroid) > 0).all()  # counter-clockwise seen from outside
    assert (np.einsum("ij,ij->i", v[:, 3:6], v[:, :3]) > 0).all()  # Hermite normals point outward


def test_demo_sdf_mesh_is_closed_and_postproc_fills_materials(pkg, oracle):
    prm = pkg.default_params()
    v, idx = pkg.mesh_extract(prm, 48)
    MR.manifold_edges(idx.cpu().numpy().astype(np.int64))
    before = v.clone()
    pkg.mesh_postproc(prm, v)
    want = oracle.mesh_postproc(oracle.params_from(prm), before.cpu().numpy())
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (v[:, 6:9].cpu().numpy() > 0).any()


def test_empty_surface_bad_algorithm_and_limits(pkg):
    import ctypes as C
    prm = pkg.default_params(sphere_radius=5.0)
    v, idx = pkg.mesh_extract(prm, 8, sdf_id=2)  # everything inside: no crossing
    assert v.shape == (0, 12) and idx.shape == (0,)
    m = pkg._capi.Mesh()
    lo, hi = pkg.f3((-1, -1, -1)), pkg.f3((1, 1, 1))
    assert pkg.lib.sdfv_mesh_extract(C.byref(prm), 0, lo, hi, 8, 3, C.byref(m), None) == -1
    assert b"Unsupported algorithm" in pkg.lib.sdfv_last_error()
    assert pkg.lib.sdfv_mesh_extract(C.byref(prm), 0, lo, hi, 0, 0, C.byref(m), None) == -1
    assert pkg.lib.sdfv_mesh_extract(C.byref(prm), 0, lo, hi, 4096, 0, C.byref(m), None) == -1
    assert pkg.lib.sdfv_mesh_free(C.byref(m)) == 0 and pkg.lib.sdfv_mesh_free(None) == 0


def test_large_lattice_counts(pkg):
    """512^3 cells: 135 M lattice points through both scans; the sphere's triangle count scales with area."""
    prm = pkg.default_params(sphere_radius=0.8)
    v, idx = pkg.mesh_extract(prm, 512, sdf_id=2)
    tri = idx.shape[0] // 3
    assert v.shape[0] - tri * 3 // 2 + tri == 2  # closed triangle mesh: E = 3F/2
    area_cells = 4 * np.pi * (0.8 * 256) ** 2
    assert 1.5 * area_cells < tri < 3.0 * area_cells


def test_scratch_is_reused_and_can_be_trimmed(pkg):
    prm = pkg.default_params()
    a = pkg.mesh_extract(prm, 40)
    free_before = torch.cuda.mem_get_info()[0]
    b = pkg.mesh_extract(prm, 24)          # smaller: runs inside the kept scratch
    assert torch.cuda.mem_get_info()[0] >= free_before - (8 << 20)
    c = pkg.mesh_extract(prm, 40)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and b[0].shape[0] < a[0].shape[0]
    assert pkg.lib.sdfv_mesh_trim() == 0 and pkg.lib.sdfv_mesh_trim() == 0
    d = pkg.mesh_extract(prm, 40)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])


def test_marching_cubes_is_the_same_before_and_after_dual_contouring(pkg):
    """The cube child at 9 cells in the non-cubic box of test_extraction_matches_numpy_restatement, algorithm 0, then 4, then 0 on
    one thread: the two meshers share the thread's scratch and the positions kernel, which writes into the output vertices for
    one and into a temporary for the other.  Guards the state shared between calls; tests/test_gpu_dual_contour.py checks what
    algorithm 4 itself returns."""
    prm = pkg.default_params(cube_half_side=0.6)
    box = ((-1.0, -0.75, -1.25), (1.0, 1.0, 0.5))

    def extract(algorithm):
        return [x.cpu().numpy() for x in pkg.mesh_extract(prm, 9, *box, sdf_id=1, algorithm=algorithm)]
    before = extract(0)
    dual = extract(4)
    after = extract(0)
    assert before[0].shape[0] > 0 and before[1].shape[0] > 0 and dual[0].shape[0] > 0 and dual[1].shape[0] > 0
    for a, b in zip(before, after):
        assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def test_randomised_extractions_match_numpy_restatement(pkg, oracle):
    """Seeded sweep (tools/soak.sh varies the seed): random demo parameters, sub-trees, boxes and lattice sizes."""
    rng = np.random.default_rng(int(os.environ.get("SDFV_SOAK_SEED", 11)))
    for _ in range(int(os.environ.get("SDFV_SOAK_TRIALS", 4))):
        kw = dict(cube_half_side=float(np.float32(rng.uniform(0.2, 1.0))), sphere_radius=float(np.float32(rng.uniform(0.2, 1.2))),
                  disable_sphere=int(rng.integers(0, 4) == 0))
        lo = rng.uniform(-1.4, -0.6, size=3).astype(np.float32)
        hi = (lo + rng.uniform(1.2, 2.8, size=3)).astype(np.float32)
        box = (tuple(float(x) for x in lo), tuple(float(x) for x in hi))
        n, sdf_id = int(rng.integers(3, 14)), int(rng.integers(0, 3))
        prm = pkg.default_params(**kw)
        v, idx = pkg.mesh_extract(prm, n, *box, sdf_id=sdf_id)
        want_v, want_i, _ = DM.extract_demo(oracle, oracle.params_from(prm), n, box, sdf_id)
        assert v.shape[0] == want_v.shape[0], (kw, box, n, sdf_id)
        if v.shape[0]:
            np.testing.assert_array_equal(MR.bits(v.cpu().numpy()[:, :3]), MR.bits(want_v[:, :3]))
            np.testing.assert_array_equal(idx.cpu().numpy().astype(np.int64), want_i)
