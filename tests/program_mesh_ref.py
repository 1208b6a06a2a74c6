"""Shared by tests/test_program_mesh_cpu.py and tests/test_gpu_program_mesh.py: a numpy float32 restatement of the mesh pipeline
over SDF programs, written from include/sdfgrid.h ("SDF programs: meshing") and calling nothing of the library.

* lattice distances: tests/program_ref.run(ops, pts, True) at u * size + min, u = (float)i / (float)cells;
* extraction: one vertex per crossing +axis edge in lattice order (x fastest) then axis order, t = d0 / (d0 - d1); triangles by
  the conventions of tools/gen_mc_table.py (its build(), not the generated .inc), cell by cell, x fastest;
* normals: normal_default_impl, the four taps and the sums in the header's order, one float32 operation per step;
* postproc: columns 1..6 of run(ops, positions, False); the normal recomputed only where |n|^2 < 1e-4.
Every arithmetic step is one numpy float32 operation on float32 operands."""
import functools
import importlib.util
import os
from collections import Counter

import numpy as np

import program_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def mc_table():
    """(tri_count [256], tri_edges [256, 15] with -1 padding) from tools/gen_mc_table.build()."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.build()
    width = 3 * max(len(t) for t in table)
    count = np.array([len(t) for t in table], np.int64)
    edges = np.full((256, width), -1, np.int64)
    for case, tris in enumerate(table):
        flat = [e for t in tris for e in t]
        edges[case, :len(flat)] = flat
    return count, edges


def lattice(ops, n, bb):
    """(axes: three [n + 1] arrays of world coordinates, d: [k, j, i] distances) of the n-cell lattice over bb = min.xyz + max.xyz."""
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    unit = np.arange(n + 1, dtype=F) / F(n)
    axes = [unit * size[a] + lo[a] for a in range(3)]
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    pts = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(F)
    d = R.run(ops, pts, True)[:, 0].reshape(n + 1, n + 1, n + 1)
    return unit, d


@np.errstate(all="ignore")
def normals(ops, p, eps=0.0):
    """normal_default_impl at p [m, 3] -> [m, 3] float32."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    e = F(eps) if eps > 0 else F(0.001)
    me = F(-1.0) * e
    x, y, z = p[:, 0], p[:, 1], p[:, 2]

    def dist(ox, oy, oz):
        return R.run(ops, np.stack([x + ox, y + oy, z + oz], axis=-1), True)[:, 0]

    d1, d2, d3, d4 = dist(e, me, me), dist(me, e, me), dist(me, me, e), dist(e, e, e)
    vx = d1 + -d2 + -d3 + d4
    vy = -d1 + d2 + -d3 + d4
    vz = -d1 + -d2 + d3 + d4
    inv = F(1.0) / np.sqrt(vx * vx + vy * vy + vz * vz)
    return np.stack([vx * inv, vy * inv, vz * inv], axis=-1).astype(F)


def extract(ops, n, bb, materials=False):
    """-> (vertices [V, 12] float32, indices [3 * T] int64, d): what sdfv_program_mesh_extract leaves for n cells over bb."""
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    unit, d = lattice(ops, n, bb)
    assert not np.isnan(d).any() and not (d == 0).any(), "the cases of the tests keep clear of exact zeros and NaNs"
    inside = d < 0
    np1 = n + 1
    # crossing flags per point and axis, [k, j, i, a]
    cross = np.zeros((np1, np1, np1, 3), bool)
    cross[:, :, :-1, 0] = inside[:, :, 1:] != inside[:, :, :-1]
    cross[:, :-1, :, 1] = inside[:, 1:, :] != inside[:, :-1, :]
    cross[:-1, :, :, 2] = inside[1:, :, :] != inside[:-1, :, :]
    flat = cross.reshape(-1)                              # lattice order (x fastest), then axis order
    vid = np.cumsum(flat) - 1                             # vertex id of (point, axis) where flat
    where = np.nonzero(flat)[0]
    point, axis = where // 3, where % 3
    i, r = point % np1, point // np1
    j, k = r % np1, r // np1
    idx = np.stack([i, j, k], axis=-1)
    nb = idx.copy()
    nb[np.arange(len(where)), axis] += 1
    d0 = d[k, j, i]
    d1 = d[nb[:, 2], nb[:, 1], nb[:, 0]]
    with np.errstate(all="ignore"):
        t = d0 / (d0 - d1)
    u = unit[idx].astype(F)                               # [V, 3]
    rows = np.arange(len(where))
    ua = u[rows, axis]
    u1 = unit[idx[rows, axis] + 1]
    u[rows, axis] = ua + t * (u1 - ua)
    pos = (u * size[None, :] + lo[None, :]).astype(F)
    # triangles
    count, edges = mc_table()
    case = np.zeros((n, n, n), np.int64)
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[cz:cz + n, cy:cy + n, cx:cx + n].astype(np.int64) << c
    case = case.reshape(-1)
    cells = np.nonzero(count[case])[0]
    tris = []
    vid3 = vid.reshape(np1, np1, np1, 3)
    for c in cells:                                       # surface cells only: O(n^2)
        ci, cr = c % n, c // n
        cj, ck = cr % n, cr // n
        for e in edges[case[c], :3 * count[case[c]]]:
            a, s = divmod(int(e), 4)
            others = [b for b in range(3) if b != a]
            owner = [ci, cj, ck]
            owner[others[0]] += s & 1
            owner[others[1]] += s >> 1
            assert cross[owner[2], owner[1], owner[0], a]
            tris.append(vid3[owner[2], owner[1], owner[0], a])
    v = np.zeros((len(where), 12), F)
    v[:, :3] = pos
    if len(where):
        v[:, 3:6] = normals(ops, pos)
        if materials:
            v[:, 6:] = R.run(ops, pos, False)[:, 1:7]
    return v, np.array(tris, np.int64), d


def postproc(ops, vertices):
    """Mesh::postproc of [m, 12] vertices -> a new array."""
    v = np.array(vertices, F, copy=True)
    if len(v) == 0:
        return v
    nx, ny, nz = v[:, 3] - F(0), v[:, 4] - F(0), v[:, 5] - F(0)
    unset = nx * nx + ny * ny + nz * nz < F(0.0001)
    if unset.any():
        v[unset, 3:6] = normals(ops, v[unset, :3])
    v[:, 6:] = R.run(ops, v[:, :3], False)[:, 1:7]
    return v


def manifold_edges(indices):
    """Asserts a closed, consistently oriented 2-manifold; returns its number of undirected edges."""
    tri = np.asarray(indices).reshape(-1, 3)
    directed = Counter()
    for a, b, c in tri:
        for e in ((a, b), (b, c), (c, a)):
            directed[e] += 1
    assert all(cnt == 1 for cnt in directed.values()), "an oriented edge is used twice"
    assert all((b, a) in directed for (a, b) in directed), "an edge has no opposite partner: the mesh is open"
    return len(directed) // 2


def assert_sphere_properties(v, idx, n, radius=0.6):
    """`single` (sphere 0.6) at n cells: closed oriented 2-manifold, Euler characteristic 2, outward faces and normals, and
    every |r - radius| < (2 / n)^2 -- linear interpolation of an exact distance over cells of side 2 / n is O(h^2) off the sphere
    (the bound and reasoning of tests/test_gpu_mesh_extract.py)."""
    v, idx = np.asarray(v), np.asarray(idx).astype(np.int64)
    assert v.shape[0] > 0 and idx.shape[0] > 0
    n_edges = manifold_edges(idx)
    assert v.shape[0] - n_edges + idx.shape[0] // 3 == 2
    assert idx.min() == 0 and idx.max() == v.shape[0] - 1 and len(np.unique(idx)) == v.shape[0]
    r = np.linalg.norm(v[:, :3].astype(np.float64), axis=1)
    assert np.abs(r - radius).max() < (2.0 / n) ** 2
    tri = v[idx.reshape(-1, 3), :3].astype(np.float64)
    face_n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", face_n, tri.mean(axis=1)) > 0).all()
    assert (np.einsum("ij,ij->i", v[:, 3:6].astype(np.float64), v[:, :3].astype(np.float64)) > 0).all()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
