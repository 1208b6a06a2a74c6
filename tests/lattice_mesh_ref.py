"""Shared by tests/test_lattice_mesh_cpu.py and tests/test_gpu_lattice_mesh.py: a numpy float32 restatement of meshing a sampled
lattice (include/sdfgrid.h, "Meshing a sampled lattice"), written from the header and calling nothing of the library.

* normals(d, bb, p): the header's eight steps -- central differences of the lattice (one-sided at the border), each component
  interpolated over the 8 corners of the cell along x, then y, then z, scaled to world units and normalised; a gradient whose
  squared length is not > 0 gives the zero normal;
* extract(d, bb, algorithm): the extraction of tests/program_mesh_ref.py and tests/dual_contour_ref.py from GIVEN distances
  d[k, j, i] instead of a program's: the crossing edges, their positions and dual contouring's solve are those modules' own
  functions, the triangles follow tools/gen_mc_table.py's table; normals from the lattice; material fields zero.
Every arithmetic step is one numpy float32 operation on float32 operands."""
import numpy as np

import dual_contour_ref as D
import program_mesh_ref as M

F = np.float32
DUAL = D.DUAL
assert_closed_and_oriented = D.assert_closed_and_oriented
assert_sphere_properties = M.assert_sphere_properties
bits = M.bits


def lerp(a, b, t):
    return a + t * (b - a)


def lattice_points(n, bb):
    """[(n + 1)^3, 3] positions in flat order (x fastest): (float)i / (float)n * size + min per axis."""
    _, _, _, axes = D.axes_of(n, bb)
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(F)


@np.errstate(all="ignore")
def normals(d, bb, p):
    """The header's normal(p) over the lattice d [k, j, i] of the box bb = min.xyz + max.xyz, at p [m, 3] -> [m, 3] float32."""
    d = np.ascontiguousarray(d, F)
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    n = d.shape[0] - 1
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    cells = F(n)
    c, f = [], []
    for a in range(3):
        u = (p[:, a] - lo[a]) / size[a] * cells                          # 1
        u = np.where(u > 0, u, F(0))
        u = np.where(u < cells, u, cells)
        ca = np.minimum(np.floor(u).astype(np.int64), n - 1)            # 2
        c.append(ca)
        f.append(u - ca.astype(F))

    def gradient(a, q):                                                  # 3
        hi, low = np.minimum(q[a] + 1, n), np.maximum(q[a], 1) - 1
        qh, ql = list(q), list(q)
        qh[a], ql[a] = hi, low
        return (d[qh[2], qh[1], qh[0]] - d[ql[2], ql[1], ql[0]]) / (hi - low).astype(F)

    G = []
    for a in range(3):
        g = {(ox, oy, oz): gradient(a, [c[0] + ox, c[1] + oy, c[2] + oz]) for oz in (0, 1) for oy in (0, 1) for ox in (0, 1)}
        x = {(oy, oz): lerp(g[0, oy, oz], g[1, oy, oz], f[0]) for oz in (0, 1) for oy in (0, 1)}      # 4
        y = {oz: lerp(x[0, oz], x[1, oz], f[1]) for oz in (0, 1)}
        G.append(lerp(y[0], y[1], f[2]) * (cells / size[a]))            # 5
    s = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]                        # 6
    inv = F(1.0) / np.sqrt(s)                                            # 8
    set_ = s > 0                                                         # 7
    return np.stack([np.where(set_, G[a] * inv, F(0)) for a in range(3)], axis=-1).astype(F)


def triangles(d):
    """Marching cubes' indices over d [k, j, i]: cell by cell (x fastest), the table's edges looked up among the crossing
    edges' vertex ids."""
    n = d.shape[0] - 1
    inside = d < 0
    cross, vid = D.crossings(d)
    count, edges = M.mc_table()
    case = np.zeros((n, n, n), np.int64)
    for corner in range(8):
        cx, cy, cz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        case |= inside[cz:cz + n, cy:cy + n, cx:cx + n].astype(np.int64) << corner
    case = case.reshape(-1)
    out = []
    for cell in np.nonzero(count[case])[0]:
        ci, r = cell % n, cell // n
        cj, ck = r % n, r // n
        for e in edges[case[cell], :3 * count[case[cell]]]:
            a, s = divmod(int(e), 4)
            o0, o1 = [b for b in range(3) if b != a]
            owner = [ci, cj, ck]
            owner[o0] += s & 1
            owner[o1] += s >> 1
            assert cross[owner[2], owner[1], owner[0], a]
            out.append(vid[owner[2], owner[1], owner[0], a])
    return np.array(out, np.int64), case


def extract(d, bb, algorithm=0):
    """What sdfv_lattice_mesh_extract leaves for the lattice d [k, j, i] over bb -> (vertices [V, 12] float32, indices int64,
    info: dict(cases = the cube case of every cell) for marching cubes, dual_contour_ref.solve()'s dict for dual contouring)."""
    d = np.ascontiguousarray(d, F)
    assert not np.isnan(d).any() and not (d == 0).any(), "the cases of the tests keep clear of exact zeros and NaNs"
    hp = D.hermite_positions(d, bb)
    if algorithm == DUAL:
        h = np.zeros((len(hp), 6), F)
        h[:, :3] = hp
        if len(hp):
            h[:, 3:6] = normals(d, bb, hp)
        info = D.solve(d, bb, h)
        info["hermite"] = h
        pos, idx = info["pos"], info["idx"]
    else:
        assert algorithm == 0
        idx, case = triangles(d)
        pos, info = hp, dict(cases=case)
    v = np.zeros((len(pos), 12), F)
    v[:, :3] = pos
    if len(pos):
        v[:, 3:6] = normals(d, bb, pos)
    return v, idx, info


def sphere_lattice(n, bb, radius=0.6):
    """d [k, j, i]: the exact distance to a sphere about the origin, rounded to float32, at the lattice points."""
    p = lattice_points(n, bb).astype(np.float64)
    return (np.linalg.norm(p, axis=1) - radius).astype(F).reshape(n + 1, n + 1, n + 1)


def gyroid_lattice(n, bb, scale=4.0, level=0.1):
    """sin x cos y + sin y cos z + sin z cos x - level at `scale` times the lattice points: a surface that cuts every face of the box."""
    p = lattice_points(n, bb).astype(np.float64) * scale
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    g = np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x) - level
    return g.astype(F).reshape(n + 1, n + 1, n + 1)
