"""CPU tests of what a mesh MEANS: the numpy restatements of every mesh route (tests/program_mesh_ref.py, tests/demo_mesh_ref.py,
tests/lattice_mesh_ref.py) against the float64 statements M1 .. M7 of tests/mesh_geometry.py, which know a distance function
and no mesh; the reference's own normals against normals known by construction; and meshes falsified on purpose, each of which
its own statement must report and none before it.  Every figure is printed.  No device needed.

M1 on the lattice, M2 a true crossing, M3 on the surface, M4 complete, M5 closed, oriented, outward, M6 normals, M7 materials:
DESIGN section 4, "What a mesh means"."""
import functools
import importlib

import numpy as np
import pytest

import demo_geometry as DG
import demo_mesh_ref as DM
import lattice_mesh_ref as LM
import mesh_geometry as MG
import program_geometry as G
import program_mesh_ref as M

F = np.float32
BB = MG.UNIT_BOX
MODELS = MG.models()


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@functools.lru_cache(maxsize=None)
def restated(name, n, algorithm):
    """The restatement's mesh of a model with materials: computed once, shared, never modified."""
    PM = importlib.import_module("sdf-viewer_amd.program")
    ops = tuple(G.emit(MODELS[name][0], PM, BB).ops)
    v, i, _ = M.extract(ops, n, BB, materials=True, algorithm=algorithm, zeros_ok=True)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


@pytest.mark.parametrize("algorithm", [0, MG.DUAL])
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_program_restatement_means_its_model(pkg, PM, name, n, algorithm):
    scene, chi = MODELS[name]
    v, i = restated(name, n, algorithm)
    field = MG.ProgramField(scene, n, BB)
    rep = MG.check_mesh(v, i, n, BB, field, algorithm, True, chi=chi)
    MG.assert_mesh(f"program_mesh_ref, {name}, {n} cells, algorithm {algorithm}, L = {field.L:.3f}, inside the box: {field.inside_box}", rep)
    if name == "sixteen":
        # cut by the plane 0.95 - z <= 0: nothing of it lies in the unit box
        assert len(v) == 0 and len(i) == 0 and rep.figures["M4 decided crossing edges"] == 0
    else:
        assert len(v) > 100 and rep.figures["M4 decided crossing edges"] > 100
    if chi is not None:
        assert field.inside_box and (algorithm == MG.DUAL or rep.figures["Euler characteristic"] == chi)


def test_the_plane_of_rotated_solids_needs_its_own_lipschitz_constant(pkg, PM):
    """|n| = 1.29 for its plane: with L = 1 the bracket M3 does not hold there, with the scene's own L it does."""
    scene, _ = MODELS["rotated_solids"]
    v, i = restated("rotated_solids", 16, 0)
    field = MG.ProgramField(scene, 16, BB)
    assert abs(field.L - float(np.linalg.norm([0.6, -0.3, 1.1]))) < 1e-6
    assert "M3" not in MG.check_mesh(v, i, 16, BB, field, 0, True, statements=("M1", "M3")).failures
    field.L = 1.0
    assert "M3" in MG.check_mesh(v, i, 16, BB, field, 0, True, statements=("M1", "M3")).failures


@pytest.mark.parametrize("algorithm", [0, MG.DUAL])
@pytest.mark.parametrize("sdf_id", [0, 1, 2])
def test_the_demo_restatement_means_the_demo(pkg, oracle, sdf_id, algorithm):
    n = 24
    prm = pkg.default_params()
    v, i, _ = DM.extract_demo(oracle, oracle.params_from(prm), n, (BB[:3], BB[3:]), sdf_id, algorithm)
    field = MG.DemoField(DG.Params(), sdf_id, n, BB)
    rep = MG.check_mesh(v, i, n, BB, field, algorithm, False, chi=2 if sdf_id == 1 else None)
    MG.assert_mesh(f"demo_mesh_ref, sdf {sdf_id}, {n} cells, algorithm {algorithm}, inside the box: {field.inside_box}", rep)
    assert len(v) > 500 and field.inside_box == (sdf_id != 2)


@pytest.mark.parametrize("algorithm", [0, MG.DUAL])
@pytest.mark.parametrize("name", ["oblique torus", "every_opcode", "rotated_solids"])
def test_the_lattice_restatement_means_the_model_it_was_sampled_from(name, algorithm):
    """The lattice route fed the float64 distances rounded to f32: M1 .. M5 (its normals are central differences of the lattice,
    another definition, and stay held to the restatement)."""
    n = 16
    scene, chi = MODELS[name]
    field = MG.ProgramField(scene, n, BB)
    d = field.evaluate(MG.lattice_positions(MG.tables(n, BB)))[0].astype(F).reshape(n + 1, n + 1, n + 1)
    v, i, _ = LM.extract(d, BB, algorithm, zeros_ok=True)
    rep = MG.check_mesh(v, i, n, BB, field, algorithm, False, chi=chi, statements=MG.NO_NORMALS)
    MG.assert_mesh(f"lattice_mesh_ref, {name}, {n} cells, algorithm {algorithm}", rep)
    assert len(v) > 100 and (v[:, 6:] == 0).all()


# ---- the reference checks itself ----
def test_tetra_normal_agrees_with_the_normals_known_by_construction():
    """At surface point + t * outward normal the level set's normal is that normal.  tetra_normal's four taps see the level set's
    curvature: the cited derivation's term, sqrt(3) e / (2 rho) (1 + sqrt(3) e / (2 rho))^2 with rho the smallest radius of
    curvature of the level set through the point (inf on a flat piece), on top of tol_sin.  Points whose taps could leave their
    smooth piece (margin <= 2 e > sqrt(3) e) are left out."""
    rng = np.random.default_rng(7)
    e = 0.001
    worst, count = 0.0, 0
    for prim in G.KNOWN_PRIMS:
        for feature, (p, _, _, normal, margin, rho) in G.known_points(prim, rng, 1024, with_normals=True).items():
            p32 = p.astype(F)
            moved = np.linalg.norm(p32.astype(np.float64) - p, axis=1)
            ok = margin > 2.0 * e + moved
            assert ok.sum() >= 400, (prim.kind, feature, int(ok.sum()))
            n, tol, decided = G.tetra_normal(prim, p32[ok], e)
            assert decided.all(), (prim.kind, feature)
            x = np.sqrt(3.0) * e / (2.0 * np.maximum(rho[ok] - moved[ok], 1e-300))
            # (rounding the point moves the level set's normal by at most moved / rho)
            allowed = x * (1.0 + x) ** 2 + tol + moved[ok] / np.maximum(rho[ok] - moved[ok], 1e-300)
            sine = np.linalg.norm(np.cross(n, normal[ok]), axis=1)
            assert ((n * normal[ok]).sum(axis=1) > 0).all(), (prim.kind, feature, "inward")
            k = int(np.argmax(sine - allowed))
            assert (sine <= allowed).all(), (prim.kind, feature, p[ok][k], n[k], normal[ok][k], sine[k], allowed[k])
            tight = allowed < 1.0
            worst = max(worst, float((sine[tight] / allowed[tight]).max()))
            count += int(ok.sum())
    print(f"tetra_normal on {count} points of known normal: max sine / tolerance = {worst:.3f}")
    assert worst < 1.0


def test_lipschitz_of_the_scenes():
    got = {name: G.lipschitz(scene) for name, scene in G.scenes().items()}
    assert got["rotated_solids"] == pytest.approx(float(np.linalg.norm([0.6, -0.3, 1.1])), abs=1e-6)
    assert all(v == pytest.approx(1.0, abs=1e-6) for k, v in got.items() if k != "rotated_solids")
    # by the definition: sampled pairs never change faster
    rng = np.random.default_rng(3)
    for name, scene in G.scenes().items():
        p, q = rng.uniform(-1, 1, (4096, 3)).astype(F), rng.normal(0, 0.05, (4096, 3)).astype(F)
        (da, ea, _, _), (db, eb, _, _) = G.evaluate(scene, p), G.evaluate(scene, p + q)
        dist = np.linalg.norm((p + q).astype(np.float64) - p.astype(np.float64), axis=1)
        assert (np.abs(da - db) <= got[name] * dist + 1e-12).all(), name


def test_two_orders_of_one_mesh_are_the_same_set_and_a_changed_word_is_not():
    import torch
    v, i = restated("every_opcode", 16, 0)
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(v))
    rank = np.empty(len(v), np.int64)
    rank[perm] = np.arange(len(v))
    tri = rank[i.reshape(-1, 3)][rng.permutation(len(i) // 3)]
    tri = np.stack([np.roll(t, int(k)) for t, k in zip(tri, rng.integers(0, 3, len(tri)))])
    a = (torch.from_numpy(v.copy()), torch.from_numpy(i.copy()))
    b = (torch.from_numpy(v[perm].copy()), torch.from_numpy(tri.reshape(-1).astype(np.int32)))
    assert MG.same_mesh_as_a_set(*a, *b) is None
    b[0][7, 4] += 1e-6
    assert "vertex records differ" in MG.same_mesh_as_a_set(*a, *b)
    b[0][7, 4] = a[0][perm[7], 4]
    b[1][:3] = b[1][:3][[0, 2, 1]]
    assert "triangles differ" in MG.same_mesh_as_a_set(*a, *b)


# ---- falsified meshes ----
def torus16():
    v, i = restated("oblique torus", 16, 0)
    return v.copy(), i.copy(), MG.ProgramField(MODELS["oblique torus"][0], 16, BB)


def reported_first(rep, statement):
    order = [s for s in MG.ALL if s in rep.failures]
    assert order and order[0] == statement, (statement, rep.lines())


def check(v, i, field, n=16):
    return MG.check_mesh(v, i, n, BB, field, 0, True, chi=0)


def edge_of(v, n=16):
    """(axis, t, p0, p1) of every vertex of a marching-cubes mesh, from its own position"""
    tabs = MG.tables(n, BB)
    on = np.stack([np.isin(v[:, a], tabs[a]) for a in range(3)], axis=1)
    axis = (~on).argmax(axis=1)
    rows = np.arange(len(v))
    c = v[rows, axis]
    j = np.array([np.searchsorted(tabs[a], x, side="right") - 1 for a, x in zip(axis, c)])
    p0 = np.array([tabs[a][k] for a, k in zip(axis, j)])
    p1 = np.array([tabs[a][k + 1] for a, k in zip(axis, j)])
    return axis, (c.astype(np.float64) - p0) / (p1.astype(np.float64) - p0), p0, p1


def test_the_unfalsified_mesh_passes():
    v, i, field = torus16()
    assert not check(v, i, field).failures


def test_a_flipped_triangle_is_reported_by_M5():
    v, i, field = torus16()
    i[3:6] = i[3:6][[0, 2, 1]]
    reported_first(check(v, i, field), "M5")


def test_a_dropped_triangle_is_reported_by_M5():
    v, i, field = torus16()
    reported_first(check(v, np.delete(i, [9, 10, 11]), field), "M5")


def test_a_vertex_one_ulp_off_its_edge_is_reported_by_M1():
    v, i, field = torus16()
    axis, _, _, _ = edge_of(v)
    k = 17
    off = (axis[k] + 1) % 3
    v[k, off] = np.nextafter(v[k, off], F(2.0))
    reported_first(check(v, i, field), "M1")


def test_a_vertex_slid_to_one_minus_t_is_reported_by_M3():
    v, i, field = torus16()
    axis, t, p0, p1 = edge_of(v)
    k = int(np.argmax(np.abs(t - 0.5)))
    assert abs(t[k] - 0.5) > 0.4
    v[k, axis[k]] = F(p0[k] + (1.0 - t[k]) * (float(p1[k]) - float(p0[k])))
    rep = check(v, i, field)
    reported_first(rep, "M3")


def test_two_vertices_on_one_edge_are_reported_by_M1():
    v, i, field = torus16()
    axis, t, p0, p1 = edge_of(v)
    extra = v[5:6].copy()
    extra[0, axis[5]] = F(p0[5] + 0.5 * (t[5] + (1.0 if t[5] < 0.5 else 0.0)) * (float(p1[5]) - float(p0[5])))
    tri = i.copy()
    tri[np.flatnonzero(tri == 5)[0]] = len(v)              # (one triangle uses it: no vertex is idle)
    reported_first(check(np.concatenate([v, extra]), tri, field), "M1")


def test_x_and_y_swapped_is_reported_by_M2():
    v, i, field = torus16()
    v[:, [0, 1]] = v[:, [1, 0]]
    reported_first(check(v, i, field), "M2")


def test_the_lattice_read_as_texel_centres_is_reported_by_M1():
    v, i, field = torus16()
    n = 16
    u = (v[:, :3].astype(np.float64) + 1.0) / 2.0 * n        # lattice units
    v[:, :3] = ((u + 0.5) / (n + 1) * 2.0 - 1.0).astype(F)     # point i at (i + 1/2) / (n + 1), the placement of a texel centre
    reported_first(check(v, i, field), "M1")


def test_negated_normals_are_reported_by_M6():
    v, i, field = torus16()
    v[:, 3:6] = -v[:, 3:6]
    reported_first(check(v, i, field), "M6")


def test_permuted_taps_are_reported_by_M6():
    """The taps k.xyy and k.yxy exchanged (d1 <-> d2 in the header's sums): the normal's x and y change places."""
    v, i, field = torus16()
    v[:, [3, 4]] = v[:, [4, 3]]
    reported_first(check(v, i, field), "M6")


def test_materials_shifted_by_one_vertex_are_reported_by_M7():
    name = "every_opcode"
    v, i = restated(name, 16, 0)
    v = v.copy()
    field = MG.ProgramField(MODELS[name][0], 16, BB)
    assert not MG.check_mesh(v, i, 16, BB, field, 0, True).failures
    v[:, 6:] = np.roll(v[:, 6:], 1, axis=0)
    reported_first(MG.check_mesh(v, i, 16, BB, field, 0, True), "M7")
    # and a mesh that was asked for none must have none
    reported_first(MG.check_mesh(v, i, 16, BB, field, 0, False), "M7")


def test_a_crossing_edge_without_a_vertex_is_reported_by_M4():
    """A vertex merged into a neighbour (an edge collapse: the mesh stays closed and oriented, chi stays): its lattice edge still
    crosses the surface and has no vertex."""
    v, i, field = torus16()
    tri = i.reshape(-1, 3)
    for k in range(0, len(v), 7):
        t0 = tri[np.flatnonzero((tri == k).any(axis=1))[0]]
        w = int(t0[t0 != k][0])
        merged = np.where(tri == k, w, tri)
        merged = merged[(merged[:, 0] != merged[:, 1]) & (merged[:, 1] != merged[:, 2]) & (merged[:, 0] != merged[:, 2])]
        merged = np.where(merged > k, merged - 1, merged)
        rep = check(np.delete(v, k, axis=0), merged.reshape(-1), field)
        if "M5" not in rep.failures:
            break
    reported_first(rep, "M4")
    assert set(rep.failures) == {"M4"}, rep.lines()
