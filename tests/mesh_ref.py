"""The one numpy float32 restatement of mesh extraction (include/sdfgrid.h: "SDF programs: meshing", "Dual contouring", "Meshing a
sampled lattice", "Meshing a loaded grid"), written from the header and calling nothing of the library.  Everything here is
independent of the SDF: it takes a lattice of distances d [k, j, i] with (cz + 1, cy + 1, cx + 1) points over the box
bb = min.xyz + max.xyz, and two callables for what the SDF alone knows -- the test-side twin of extract_mesh's `attributes`
(sdf-viewer_amd/csrc/api_points_mesh.hip).  Wherever a cell count is taken, an int means that many cells on every axis.

* crossings, edge_positions: one vertex (or Hermite record) per crossing +axis edge, in lattice order (x fastest) then axis
  order, t = d0 / (d0 - d1);
* triangles: marching cubes by the conventions of tools/gen_mc_table.py (its build(), not the generated .inc), cell by cell;
* solve: dual contouring's mass point, normal equations, 24 steps, clamp to the cell, and quads per interior crossing edge;
* cell_of, lattice_normals: the header's normal(p) over a lattice, its eight steps numbered below;
* extract: the only orchestrator; directed_edges, manifold_edges, assert_closed_and_oriented, assert_sphere_properties: what
  any correct extractor's output has.
What is particular to an SDF kind lives in tests/program_mesh_ref.py, tests/demo_mesh_ref.py, tests/lattice_mesh_ref.py and
tests/grid_mesh_ref.py; tests/golden/mesh_ref_pins.json pins what every route returns (tests/test_mesh_ref_pins.py).

Every arithmetic step is one numpy float32 operation on float32 operands.  Sums over a cell's edges are NOT numpy reductions:
the edges are visited e = 0..11 in a Python loop and each step is an elementwise operation over all active cells, so the order
of the additions is the header's."""
import functools
import importlib.util
import os
from collections import Counter

import numpy as np

import program_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUAL = 4                                                  # SDFV_MESHER_DUAL_CONTOURING_PARTICLE


@functools.lru_cache(maxsize=None)
def mc_generator():
    """tools/gen_mc_table.py as a module: the one place that loads it."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def mc_table():
    """(tri_count [256], tri_edges [256, 15] with -1 padding) from tools/gen_mc_table.build()."""
    table = mc_generator().build()
    width = 3 * max(len(t) for t in table)
    count = np.array([len(t) for t in table], np.int64)
    edges = np.full((256, width), -1, np.int64)
    for case, tris in enumerate(table):
        flat = [e for t in tris for e in t]
        edges[case, :len(flat)] = flat
    return count, edges


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def lerp(a, b, t):
    return a + t * (b - a)


# ---- the lattice ----
def per_axis(cells):
    return (int(cells),) * 3 if np.ndim(cells) == 0 else tuple(int(c) for c in cells)


def cells_of(d):
    return (d.shape[2] - 1, d.shape[1] - 1, d.shape[0] - 1)


def axes_of(cells, bb):
    """-> (unit: three arrays (float)i / (float)cells, lo, size, axes: unit * size + lo per axis)."""
    cells = per_axis(cells)
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    unit = [np.arange(cells[a] + 1, dtype=F) / F(cells[a]) for a in range(3)]
    return unit, lo, size, [unit[a] * size[a] + lo[a] for a in range(3)]


def lattice_points(cells, bb):
    """[points, 3] positions in flat order (x fastest): (float)i / (float)cells * size + min per axis."""
    _, _, _, axes = axes_of(cells, bb)
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(F)


def crossings(d):
    """d [k, j, i] -> (cross [k, j, i, a] bool, vid [k, j, i, a]: the vertex or Hermite record of a crossing edge)."""
    inside = d < 0
    cross = np.zeros(d.shape + (3,), bool)
    cross[:, :, :-1, 0] = inside[:, :, 1:] != inside[:, :, :-1]
    cross[:, :-1, :, 1] = inside[:, 1:, :] != inside[:, :-1, :]
    cross[:-1, :, :, 2] = inside[1:, :, :] != inside[:-1, :, :]
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)
    return cross, vid


@np.errstate(all="ignore")
def edge_positions(d, bb):
    """edge_position of every crossing edge, in lattice order (x fastest) then axis order -> [E, 3]."""
    unit, lo, size, _ = axes_of(cells_of(d), bb)
    cross, _ = crossings(d)
    kk, jj, ii, aa = np.nonzero(cross)                    # C order of [k, j, i, a]: lattice order, then axis order
    idx = np.stack([ii, jj, kk], axis=-1)
    rows = np.arange(len(aa))
    nb = idx.copy()
    nb[rows, aa] += 1
    d0, d1 = d[kk, jj, ii], d[nb[:, 2], nb[:, 1], nb[:, 0]]
    t = d0 / (d0 - d1)
    u = np.stack([unit[a][idx[:, a]] for a in range(3)], axis=-1).astype(F)
    ua = u[rows, aa]
    u1 = np.array([unit[a][i + 1] for a, i in zip(aa, idx[rows, aa])], F).reshape(ua.shape)
    u[rows, aa] = ua + t * (u1 - ua)
    return (u * size[None, :] + lo[None, :]).astype(F)


def cell_owner(cells, cell, e):
    """The lattice point that owns edge e of the cells `cell` (flat, x fastest) -> ([i, j, k], axis)."""
    ci, r = cell % cells[0], cell // cells[0]
    cj, ck = r % cells[1], r // cells[1]
    a, s = divmod(int(e), 4)
    o0, o1 = [b for b in range(3) if b != a]
    owner = [ci, cj, ck]
    owner[o0] = owner[o0] + (s & 1)
    owner[o1] = owner[o1] + (s >> 1)
    return owner, a


# ---- marching cubes ----
def triangles(d):
    """Marching cubes' indices over d [k, j, i]: cell by cell (x fastest), the table's edges looked up among the crossing
    edges' vertex ids -> (indices int64, the cube case of every cell)."""
    cx, cy, cz = cells_of(d)
    inside = d < 0
    cross, vid = crossings(d)
    count, edges = mc_table()
    case = np.zeros((cz, cy, cx), np.int64)
    for corner in range(8):
        ox, oy, oz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        case |= inside[oz:oz + cz, oy:oy + cy, ox:ox + cx].astype(np.int64) << corner
    case = case.reshape(-1)
    out = []
    for cell in np.nonzero(count[case])[0]:               # surface cells only: O(n^2)
        for e in edges[case[cell], :3 * count[case[cell]]]:
            owner, a = cell_owner((cx, cy, cz), int(cell), e)
            assert cross[owner[2], owner[1], owner[0], a]
            out.append(vid[owner[2], owner[1], owner[0], a])
    return np.array(out, np.int64), case


# ---- dual contouring ----
@np.errstate(all="ignore")
def solve(d, bb, hermite):
    """d [k, j, i] float32, hermite [E, >= 6] (position, normal) -> dict(pos [V, 3], idx [6 * quads] int64, mass [V, 3],
    used [V] (the k of the header), edges [V] (the m), cells [V] flat cell ids, quads)."""
    cells = cells_of(d)
    cx, cy, cz = cells
    hermite = np.ascontiguousarray(hermite, F)
    _, _, _, axes = axes_of(cells, bb)
    cross, vid = crossings(d)
    assert hermite.shape[0] == int(cross.sum())
    all_cells = np.arange(cx * cy * cz)
    present, rec = [], []
    for e in range(12):
        owner, a = cell_owner(cells, all_cells, e)
        present.append(cross[owner[2], owner[1], owner[0], a])
        rec.append(vid[owner[2], owner[1], owner[0], a])
    active = np.any(present, axis=0)
    act = np.nonzero(active)[0]
    ci, r = act % cx, act // cx
    cj, ck = r % cy, r // cy
    present = [p[act] for p in present]
    rec = [np.where(p, r_[act], 0) for p, r_ in zip(present, rec)]
    nv = len(act)
    zero = np.zeros(nv, F)
    # mass point
    c = [zero.copy(), zero.copy(), zero.copy()]
    m = np.zeros(nv, np.int64)
    for e in range(12):
        for b in range(3):
            c[b] = np.where(present[e], c[b] + hermite[rec[e], b], c[b])
        m += present[e]
    c = [c[b] / m.astype(F) for b in range(3)]
    # normal equations
    mxx, mxy, mxz, myy, myz, mzz, gx, gy, gz = (zero.copy() for _ in range(9))
    k = np.zeros(nv, np.int64)
    for e in range(12):
        h = hermite[rec[e]]
        nx, ny, nz = h[:, 3], h[:, 4], h[:, 5]
        w = nx * nx + ny * ny + nz * nz
        used = present[e] & (w > F(0.5)) & (w < F(2.0))
        rx, ry, rz = h[:, 0] - c[0], h[:, 1] - c[1], h[:, 2] - c[2]
        b = (nx * rx + ny * ry) + nz * rz
        mxx = np.where(used, mxx + nx * nx, mxx)
        mxy = np.where(used, mxy + nx * ny, mxy)
        mxz = np.where(used, mxz + nx * nz, mxz)
        myy = np.where(used, myy + ny * ny, myy)
        myz = np.where(used, myz + ny * nz, myz)
        mzz = np.where(used, mzz + nz * nz, mzz)
        gx = np.where(used, gx + nx * b, gx)
        gy = np.where(used, gy + ny * b, gy)
        gz = np.where(used, gz + nz * b, gz)
        k += used
    s = F(1.0) / k.astype(F)
    yx, yy, yz = zero.copy(), zero.copy(), zero.copy()
    for _ in range(24):
        tx = gx - ((mxx * yx + mxy * yy) + mxz * yz)
        ty = gy - ((mxy * yx + myy * yy) + myz * yz)
        tz = gz - ((mxz * yx + myz * yy) + mzz * yz)
        yx, yy, yz = yx + s * tx, yy + s * ty, yz + s * tz
    some = k > 0
    y = [np.where(some, yx, zero), np.where(some, yy, zero), np.where(some, yz, zero)]
    pos = np.zeros((nv, 3), F)
    for b, cell in enumerate((ci, cj, ck)):
        pos[:, b] = R.pmax(axes[b][cell], R.pmin(c[b] + y[b], axes[b][cell + 1]))   # the program table's min and max
    # quads: per interior crossing edge, in the Hermite order
    cell_vertex = np.cumsum(active) - 1
    kk, jj, ii, aa = np.nonzero(cross)
    idx = np.stack([ii, jj, kk], axis=-1)
    out = []
    for row in range(len(aa)):
        a = int(aa[row])
        o0, o1 = [b for b in range(3) if b != a]
        p = idx[row]
        if not (1 <= p[o0] <= cells[o0] - 1 and 1 <= p[o1] <= cells[o1] - 1):
            continue
        q = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            cc = [int(p[0]), int(p[1]), int(p[2])]
            cc[o0] += du
            cc[o1] += dv
            flat = (cc[2] * cy + cc[1]) * cx + cc[0]
            assert active[flat]
            q.append(int(cell_vertex[flat]))
        flip = (a == 1) != bool(d[p[2], p[1], p[0]] >= 0)
        out += [q[0], q[2], q[1], q[0], q[3], q[2]] if flip else [q[0], q[1], q[2], q[0], q[2], q[3]]
    return dict(pos=pos, idx=np.array(out, np.int64), mass=np.stack(c, axis=-1).astype(F) if nv else np.zeros((0, 3), F),
                used=k, edges=m, cells=act, quads=len(out) // 6)


# ---- normals from a lattice ----
@np.errstate(all="ignore")
def cell_of(p, bb, cells):
    """Steps 1-2 of normal(p) per axis -> (c [3][m] integers, f [3][m] float32)."""
    cells = per_axis(cells)
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    c, f = [], []
    for a in range(3):
        n = F(cells[a])
        u = (p[:, a] - lo[a]) / size[a] * n                                  # 1
        u = np.where(u > 0, u, F(0))
        u = np.where(u < n, u, n)
        ca = np.minimum(np.floor(u).astype(np.int64), cells[a] - 1)         # 2
        c.append(ca)
        f.append(u - ca.astype(F))
    return c, f


@np.errstate(all="ignore")
def lattice_normals(d, bb, p):
    """The header's normal(p) over the lattice d [k, j, i] of the box bb, at p [m, 3] -> [m, 3] float32: central differences of
    the lattice (one-sided at the border), each component interpolated over the 8 corners of the cell along x, then y, then z,
    scaled to world units and normalised; a gradient whose squared length is not > 0 gives the zero normal."""
    d = np.ascontiguousarray(d, F)
    cells = cells_of(d)
    size = np.array(bb[3:], F) - np.array(bb[:3], F)
    c, f = cell_of(p, bb, cells)

    def gradient(a, q):                                                      # 3
        hi, low = np.minimum(q[a] + 1, cells[a]), np.maximum(q[a], 1) - 1
        qh, ql = list(q), list(q)
        qh[a], ql[a] = hi, low
        return (d[qh[2], qh[1], qh[0]] - d[ql[2], ql[1], ql[0]]) / (hi - low).astype(F)

    G = []
    for a in range(3):
        g = {(ox, oy, oz): gradient(a, [c[0] + ox, c[1] + oy, c[2] + oz]) for oz in (0, 1) for oy in (0, 1) for ox in (0, 1)}
        x = {(oy, oz): lerp(g[0, oy, oz], g[1, oy, oz], f[0]) for oz in (0, 1) for oy in (0, 1)}      # 4
        y = {oz: lerp(x[0, oz], x[1, oz], f[1]) for oz in (0, 1)}
        G.append(lerp(y[0], y[1], f[2]) * (F(cells[a]) / size[a]))          # 5
    s = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]                            # 6
    inv = F(1.0) / np.sqrt(s)                                                # 8
    return np.stack([np.where(s > 0, G[a] * inv, F(0)) for a in range(3)], axis=-1).astype(F)   # 7


# ---- the orchestrator ----
def extract(d, bb, algorithm, normals, materials=None, zeros_ok=False):
    """What an extraction entry point leaves for the lattice d [k, j, i] over bb.  normals(p) -> [m, 3] and materials(p) -> [m, 6]
    are the SDF's own; materials are applied to the output vertices only, never to Hermite records, as on the device.
    -> (vertices [V, 12] float32, indices int64, info): info has `lattice`; `cases` (the cube case of every cell) for marching
    cubes; solve()'s dictionary and `hermite` for dual contouring."""
    d = np.ascontiguousarray(d, F)
    # (zeros_ok: a caller that compares with no device result bit for bit -- a zero is outside, its vertex on the lattice point)
    assert not np.isnan(d).any() and (zeros_ok or not (d == 0).any()), "the cases of the tests keep clear of exact zeros and NaNs"
    hp = edge_positions(d, bb)
    info = dict(lattice=d)
    if algorithm == DUAL:
        h = np.zeros((len(hp), 6), F)
        h[:, :3] = hp
        if len(hp):
            h[:, 3:6] = normals(hp)
        info.update(solve(d, bb, h), hermite=h)
        pos, idx = info["pos"], info["idx"]
    else:
        assert algorithm == 0
        idx, info["cases"] = triangles(d)
        pos = hp
    v = np.zeros((len(pos), 12), F)
    v[:, :3] = pos
    if len(pos):
        v[:, 3:6] = normals(pos)
        if materials is not None:
            v[:, 6:] = materials(pos)
    return v, idx, info


# ---- what a correct extractor's output has ----
def directed_edges(indices):
    """-> Counter of the directed edges (a, b) of the triangles."""
    directed = Counter()
    for a, b, c in np.asarray(indices).reshape(-1, 3):
        for e in ((a, b), (b, c), (c, a)):
            directed[(int(e[0]), int(e[1]))] += 1
    return directed


def manifold_edges(indices):
    """Asserts a closed, consistently oriented 2-manifold; returns its number of undirected edges."""
    directed = directed_edges(indices)
    assert all(cnt == 1 for cnt in directed.values()), "an oriented edge is used twice"
    assert all((b, a) in directed for (a, b) in directed), "an edge has no opposite partner: the mesh is open"
    return len(directed) // 2


def assert_closed_and_oriented(indices):
    """Every directed edge occurs exactly as often as its reverse (dual contouring may use an edge twice where two sheets of the
    surface pass through one cell, so this is the multiset form of manifold_edges)."""
    directed = directed_edges(indices)
    bad = [(e, cnt, directed.get((e[1], e[0]), 0)) for e, cnt in directed.items() if directed.get((e[1], e[0]), 0) != cnt]
    assert not bad, bad[:5]


def assert_sphere_properties(v, idx, n, radius=0.6):
    """A sphere about the origin at n cells of [-1, 1]^3: closed oriented 2-manifold, Euler characteristic 2, every vertex used,
    outward faces and normals, and every |r - radius| < (2 / n)^2 -- linear interpolation of an exact distance over cells of
    side 2 / n is O(h^2) off the sphere."""
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
