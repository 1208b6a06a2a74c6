"""Shared by tests/test_dual_contour_cpu.py and tests/test_gpu_dual_contour.py: a numpy float32 restatement of dual contouring
(include/sdfgrid.h, "Dual contouring"), written from the header and calling nothing of the library.

The algorithm does not depend on the SDF: solve() takes the lattice distances and the Hermite records (position + normal per
crossing edge, in lattice order then axis order) and returns positions and indices.  The SDF-dependent parts come from what is
already pinned: for programs tests/program_ref.py (distances) and tests/program_mesh_ref.py (normals, materials); for the demo
tree tests/oracle_binding.py (source_scalar_many, normal_many).

Every arithmetic step is one numpy float32 operation on float32 operands.  Sums over a cell's edges are NOT numpy reductions:
the edges are visited e = 0..11 in a Python loop and each step is an elementwise operation over all active cells, so the order
of the additions is the header's."""
import functools

import numpy as np

import program_mesh_ref as M
import program_ref as R

F = np.float32
DUAL = 4                                                  # SDFV_MESHER_DUAL_CONTOURING_PARTICLE


def crossings(d):
    """d [k, j, i] -> (cross [k, j, i, a] bool, vid [k, j, i, a]: the Hermite record of a crossing edge)."""
    inside = d < 0
    cross = np.zeros(d.shape + (3,), bool)
    cross[:, :, :-1, 0] = inside[:, :, 1:] != inside[:, :, :-1]
    cross[:, :-1, :, 1] = inside[:, 1:, :] != inside[:, :-1, :]
    cross[:-1, :, :, 2] = inside[1:, :, :] != inside[:-1, :, :]
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)
    return cross, vid


def axes_of(n, bb):
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    unit = np.arange(n + 1, dtype=F) / F(n)
    return unit, lo, size, [unit * size[a] + lo[a] for a in range(3)]


@np.errstate(all="ignore")
def hermite_positions(d, bb):
    """edge_position of every crossing edge, in lattice order (x fastest) then axis order -> [E, 3]."""
    n = d.shape[0] - 1
    unit, lo, size, _ = axes_of(n, bb)
    cross, _ = crossings(d)
    kk, jj, ii, aa = np.nonzero(cross)                    # C order of [k, j, i, a]: lattice order, then axis order
    idx = np.stack([ii, jj, kk], axis=-1)
    nb = idx.copy()
    rows = np.arange(len(aa))
    nb[rows, aa] += 1
    d0, d1 = d[kk, jj, ii], d[nb[:, 2], nb[:, 1], nb[:, 0]]
    t = d0 / (d0 - d1)
    u = unit[idx].astype(F)
    ua, u1 = u[rows, aa], unit[idx[rows, aa] + 1]
    u[rows, aa] = ua + t * (u1 - ua)
    return (u * size[None, :] + lo[None, :]).astype(F)


@np.errstate(all="ignore")
def solve(d, bb, hermite):
    """d [k, j, i] float32, hermite [E, >= 6] (position, normal) -> dict(pos [V, 3], idx [6 * quads] int64, mass [V, 3],
    used [V] (the k of the header), edges [V] (the m), cells [V] flat cell ids, quads)."""
    n = d.shape[0] - 1
    hermite = np.ascontiguousarray(hermite, F)
    _, _, _, axes = axes_of(n, bb)
    cross, vid = crossings(d)
    assert hermite.shape[0] == int(cross.sum())
    ck, cj, ci = [x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")]
    present, rec = [], []
    for e in range(12):
        a, s = divmod(e, 4)
        o0, o1 = [b for b in range(3) if b != a]
        owner = [ci.copy(), cj.copy(), ck.copy()]
        owner[o0] = owner[o0] + (s & 1)
        owner[o1] = owner[o1] + (s >> 1)
        present.append(cross[owner[2], owner[1], owner[0], a])
        rec.append(vid[owner[2], owner[1], owner[0], a])
    active = np.any(present, axis=0)
    cells = np.nonzero(active)[0]
    ci, cj, ck = ci[cells], cj[cells], ck[cells]
    present = [p[cells] for p in present]
    rec = [np.where(p, r[cells], 0) for p, r in zip(present, rec)]
    nv = len(cells)
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
        if not (1 <= p[o0] <= n - 1 and 1 <= p[o1] <= n - 1):
            continue
        q = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            cc = [int(p[0]), int(p[1]), int(p[2])]
            cc[o0] += du
            cc[o1] += dv
            flat = (cc[2] * n + cc[1]) * n + cc[0]
            assert active[flat]
            q.append(int(cell_vertex[flat]))
        flip = (a == 1) != bool(d[p[2], p[1], p[0]] >= 0)
        out += [q[0], q[2], q[1], q[0], q[3], q[2]] if flip else [q[0], q[1], q[2], q[0], q[2], q[3]]
    return dict(pos=pos, idx=np.array(out, np.int64), mass=np.stack(c, axis=-1).astype(F) if nv else np.zeros((0, 3), F),
                used=k, edges=m, cells=cells, quads=len(out) // 6)


def extract_program(ops, n, bb, materials=False):
    """What sdfv_program_mesh_extract(algorithm = 4) leaves -> (vertices [V, 12], indices, the solve() dict)."""
    _, d = M.lattice(ops, n, bb)
    assert not np.isnan(d).any() and not (d == 0).any(), "the cases of the tests keep clear of exact zeros and NaNs"
    hp = hermite_positions(d, bb)
    h = np.zeros((len(hp), 6), F)
    h[:, :3] = hp
    if len(hp):
        h[:, 3:6] = M.normals(ops, hp)
    s = solve(d, bb, h)
    s["hermite"] = h
    v = np.zeros((len(s["pos"]), 12), F)
    v[:, :3] = s["pos"]
    if len(v):
        v[:, 3:6] = M.normals(ops, s["pos"])
        if materials:
            v[:, 6:] = R.run(ops, s["pos"], False)[:, 1:7]
    return v, s["idx"], s


def extract_demo(oracle, oprm, n, box, sdf_id=0):
    """What sdfv_mesh_extract(algorithm = 4) leaves for the demo tree, from the oracle's distances and normals."""
    ax = np.arange(n + 1, dtype=F) / F(n)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)                    # [i, j, k, 3]
    d = oracle.source_scalar_many(oprm, pts.reshape(-1, 3), box[0], box[1], sdf_id).reshape(n + 1, n + 1, n + 1)
    d = np.ascontiguousarray(d.transpose(2, 1, 0))                                     # [k, j, i]
    assert not np.isnan(d).any() and not (d == 0).any()
    bb = tuple(box[0]) + tuple(box[1])
    hp = hermite_positions(d, bb)
    h = np.zeros((len(hp), 6), F)
    h[:, :3] = hp
    if len(hp):
        h[:, 3:6] = oracle.normal_many(oprm, hp, 0.0, sdf_id)
    s = solve(d, bb, h)
    s["hermite"] = h
    v = np.zeros((len(s["pos"]), 12), F)
    v[:, :3] = s["pos"]
    if len(v):
        v[:, 3:6] = oracle.normal_many(oprm, s["pos"], 0.0, sdf_id)
    return v, s["idx"], s


def assert_closed_and_oriented(indices):
    """Every directed edge occurs exactly as often as its reverse (dual contouring may use an edge twice where two sheets of the
    surface pass through one cell, so this is the multiset form of program_mesh_ref.manifold_edges)."""
    from collections import Counter
    tri = np.asarray(indices).reshape(-1, 3)
    directed = Counter()
    for a, b, c in tri:
        for e in ((a, b), (b, c), (c, a)):
            directed[(int(e[0]), int(e[1]))] += 1
    bad = [(e, cnt, directed.get((e[1], e[0]), 0)) for e, cnt in directed.items() if directed.get((e[1], e[0]), 0) != cnt]
    assert not bad, bad[:5]


@functools.lru_cache(maxsize=None)
def primitive(kind, size):
    """ops of a one-instruction program: ("cube" | "sphere", size)."""
    return ((R.CUBE if kind == "cube" else R.SPHERE, (float(size),)),)
